"""CPU tests of the sun layer (include/meteor_demod_amd_sun.h): the sun's position against known equinoxes, solstices and the
equation of time; the gain nodes of csrc/sun_host.cpp against the numpy model of tests/sun_ref.py on map_ref.py's geolocation; the
C++ host model of the apply against sun_ref's bytes and counts; every refusal with its text and nothing written; the slot rule of
the host entry; the defaults, the workspace and the binding tables.  Every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import datetime
import re

import numpy as np
import pytest

import map_util as M
import sun_ref as S
import sun_util as U
from conftest import ROOT


def _day(text: str) -> tuple:
    t = datetime.datetime.fromisoformat(text)
    return (t.date() - datetime.date(1970, 1, 1)).days, t.hour * 3600.0 + t.minute * 60.0 + t.second


# ------------------------------------------------------------------------------------------------------------------ astronomy
@pytest.mark.parametrize("when, want", [("2024-03-20 03:06", 0.0), ("2024-09-22 12:44", 0.0), ("2024-06-20 20:51", 23.4354), ("2024-12-21 09:21", -23.4354)])
def test_declination_at_equinoxes_and_solstices(when, want):
    from meteor_demod_amd import sun
    date, utc = _day(when)
    s = sun.position(date, utc)
    dec, ref = float(np.degrees(np.arcsin(s[2]))), S.declination(date, utc)
    print(f"{when}: declination {dec:+.4f} (sun_ref {ref:+.4f}), wanted {want:+.4f}")
    assert abs(np.linalg.norm(s) - 1.0) < 1e-12
    assert abs(dec - want) < 0.02 and abs(ref - want) < 0.02 and abs(dec - ref) < 1e-9


@pytest.mark.parametrize("when, want", [("2024-11-03 12:00", -4.111), ("2024-02-11 12:00", 3.550)])
def test_subsolar_longitude_at_noon(when, want):
    from meteor_demod_amd import sun
    date, utc = _day(when)
    s = sun.position(date, utc)
    lon, ref = float(np.degrees(np.arctan2(s[1], s[0]))), S.subsolar_longitude(date, utc)
    print(f"{when}: sub-solar longitude {lon:+.4f} (sun_ref {ref:+.4f}), wanted {want:+.4f}")
    assert abs(lon - want) < 0.05 and abs(ref - want) < 0.05 and abs(lon - ref) < 1e-9


def test_cos_zenith_at_the_subsolar_point_and_its_antipode():
    from meteor_demod_amd import sun
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(50):
        date, utc = int(rng.integers(15000, 25000)), float(rng.uniform(-40000.0, 130000.0))
        s = sun.position(date, utc)
        lat, lon = np.degrees(np.arcsin(s[2])), np.degrees(np.arctan2(s[1], s[0]))
        c = sun.cos_zenith(date, [utc, utc, utc], [lat, -lat, 0.0], [lon, lon + 180.0, lon + 90.0])
        r = S.cos_zenith(date, utc, np.array([lat, -lat, 0.0]), np.array([lon, lon + 180.0, lon + 90.0]))
        worst = max(worst, abs(c[0] - 1.0), abs(c[1] + 1.0), abs(c[2]), float(np.abs(c - r).max()))
    print(f"cos z at the sub-solar point, its antipode and a quarter turn away: worst error {worst:.2e}")
    assert worst < 1e-12
    # a time of day beyond the day is the next day's, and an array of times broadcasts against the coordinates
    a = sun.cos_zenith(20000, 86400.0 + 3600.0, [10.0, 50.0], [20.0, -70.0])
    b = sun.cos_zenith(20001, 3600.0, [10.0, 50.0], [20.0, -70.0])
    assert np.abs(a - b).max() < 1e-12 and np.isnan(sun.cos_zenith(20000, [np.nan], [0.0], [0.0])).all()


# ---------------------------------------------------------------------------------------------------------------------- nodes
NODE_CASES = [("day", 77, 85.0, 45.0, None), ("terminator", 77, 85.0, 45.0, None), ("terminator", 40, 60.0, 0.0, None), ("terminator", 3, 89.0, 80.0, None),
              ("day", 1, 85.0, 45.0, None), ("day", 30, 85.0, 45.0, 130.0)]


@pytest.mark.parametrize("name, rows, limit, ref, scan", NODE_CASES, ids=lambda v: str(v))
def test_nodes_equal_the_numpy_model(name, rows, limit, ref, scan):
    from meteor_demod_amd import sun
    opts = U.map_opts(name)
    if scan is not None:
        opts["scan_deg"] = scan
    gain, summ = sun.nodes(M.tle_text(), U.timing(name, rows), rows, limit_deg=limit, ref_deg=ref, **opts)
    want, real, c = U.ref_nodes(name, rows, limit, ref, scan)
    there = want != S.NO_NODE
    diff = np.abs(gain[there].astype(np.int64) - want[there].astype(np.int64))
    z = np.degrees(np.arccos(np.clip(c[there], -1.0, 1.0)))
    print(f"{name} rows {rows} limit {limit} ref {ref} scan {scan}: zenith {summ['zenith_min']:.3f} .. {summ['zenith_max']:.3f} (sun_ref {z.min():.3f} .. {z.max():.3f}), "
          f"{summ['missing']} of {summ['nodes']} missing, {summ['at_limit']} at the limit, largest |dG| {diff.max()}, {int((diff > 0).sum())} nodes differ, largest G {gain[there].max()}")
    assert gain.shape == want.shape == (rows + 1, 99) and gain.dtype == np.uint32
    assert np.array_equal(gain == S.NO_NODE, ~there)
    assert diff.max() <= 1 and (diff > 0).sum() <= 3                               # only a rounding tie can differ
    assert gain[there].max() < 1 << 22
    assert summ["nodes"] == gain.size and summ["missing"] == int((~there).sum()) and summ["slot_mask"] == 0 and summ["saturated"] == [0, 0, 0]
    assert summ["at_limit"] == int((c[there] < np.cos(np.radians(limit))).sum()) and summ["date"] == opts["date"]
    assert abs(summ["zenith_min"] - z.min()) < 1e-6 and abs(summ["zenith_max"] - z.max()) < 1e-6
    if scan == 130.0:
        assert 0 < summ["missing"] < gain.size // 4 and not there[:, 0].any() and there[:, 49].all()
    else:
        assert summ["missing"] == 0


def test_the_passes_are_what_their_names_say():
    lo, hi = S.zenith_range(U.ref_pass("day"), U.ROWS)
    print(f"day: {lo:.2f} .. {hi:.2f}")
    assert hi < 70.0
    lo, hi = S.zenith_range(U.ref_pass("terminator"), U.ROWS)
    print(f"terminator: {lo:.2f} .. {hi:.2f}")
    assert lo < 80.0 and hi > 95.0
    # the gain at the reference angle is 1, and a node beyond the limit has the limit's gain
    assert S.nodes(U.ref_pass("day"), 1, 85.0, 45.0)[0].min() > 65536 * np.cos(np.radians(45.0)) / 1.0 - 1
    g, _, c = U.ref_nodes("terminator")
    assert (g[c < np.cos(np.radians(85.0))] == int(np.floor(65536 * np.cos(np.radians(45.0)) / np.cos(np.radians(85.0)) + 0.5))).all()


# ---------------------------------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("rows", [1, 3, 77])
def test_model_equals_numpy_model(rows):
    from meteor_demod_amd import sun
    pics = U.pictures(rows)
    n = changed = 0
    for kind in ("day", "terminator", "synthetic"):
        gain = U.gain_table(kind, rows)
        for mask in (1, 2, 5, 7):
            out, sat = sun.model_apply(pics, gain, mask)
            want, wsat = S.apply(pics, gain, mask)
            for k in range(3):
                if mask >> k & 1:
                    assert np.array_equal(out[k], want[k]), (rows, kind, mask, k)
                    changed += int((out[k] != pics[k]).sum())
                else:
                    assert out[k] is pics[k]
            assert sat == wsat and all(sat[k] == 0 for k in range(3) if not mask >> k & 1), (rows, kind, mask, sat, wsat)
            print(f"rows {rows} {kind} mask {mask}: saturated {sat}")
            n += 1
    assert n == 12 and changed > 0


def test_model_properties():
    """A gain of 1 changes nothing; zeroes stay zero under any gain; a cell with a missing corner is copied; in place equals out of
    place."""
    from meteor_demod_amd import sun
    rows = 3
    pics = U.pictures(rows)
    one = np.full((rows + 1, 99), 65536, np.uint32)
    out, sat = sun.model_apply(pics, one, 7)
    assert all(np.array_equal(out[k], pics[k]) for k in range(3)) and sat == [0, 0, 0]
    gain = U.synthetic_gain(rows)
    out, sat = sun.model_apply(pics, gain, 7)
    _, missing = S.pixel_gain(gain, rows)
    assert 0.2 < missing.mean() < 0.9
    # every edge of a cell: the cells made by hand lack exactly one corner and are copied whole
    for a, b in ((0, 3), (0, 6), (rows - 1, 9), (rows - 1, 12), (rows // 2, 97)):
        cell = (slice(8 * a, 8 * a + 8), slice(16 * b, 16 * b + 16))
        assert missing[cell].all()
    for k in range(3):
        assert np.array_equal(out[k][missing], pics[k][missing]) and not out[k][pics[k] == 0].any()
    # in place, through the C entry itself
    same = [p.copy() for p in pics]
    ptr, sat2 = (C.c_void_p * 3)(*[p.ctypes.data for p in same]), (C.c_uint64 * 3)()
    assert sun.lib().mdemod_sun_model_apply(C.byref(ptr), C.byref(ptr), 7, rows, gain.ctypes.data, C.byref(sat2)) == 0
    assert all(np.array_equal(same[k], out[k]) for k in range(3)) and list(sat2) == sat
    print(f"{missing.mean():.2f} of the pixels under a missing corner; saturated {sat}")


# ------------------------------------------------------------------------------------------------------------------- refusals
def _refused(code, pattern):
    from meteor_demod_amd import _capi
    text = _capi.last_error()
    print(f"  {code}: {text}")
    assert code == -1 and re.search(pattern, text), (code, text)


def test_model_apply_refusals_write_nothing():
    from meteor_demod_amd import sun
    L = sun.lib()
    rows = 2
    pics = U.pictures(rows)
    big = np.full(4 * 8 * rows * 1568 + 8, 0xA5, np.uint8)                            # room for three outputs and a misaligned one
    area = 8 * rows * 1568
    gain = U.synthetic_gain(rows)
    sat = (C.c_uint64 * 3)(7, 7, 7)

    def call(image, out, mask, rows_, g):
        pi, po = (C.c_void_p * 3)(*image), (C.c_void_p * 3)(*out)
        return L.mdemod_sun_model_apply(C.byref(pi), C.byref(po), mask, rows_, g, C.byref(sat))
    im = [p.ctypes.data for p in pics]
    o = [big.ctypes.data + k * area for k in range(3)]
    assert pics[0].ctypes.data % 4 == 0 and big.ctypes.data % 4 == 0
    _refused(call(im, o, 7, 0, gain.ctypes.data), r"0 strip rows are outside 1 \.\. 8192")
    _refused(call(im, o, 7, 8193, gain.ctypes.data), r"8193 strip rows are outside 1 \.\. 8192")
    _refused(call(im, o, 0, rows, gain.ctypes.data), r"slot mask 0 is outside 1 \.\. 7")
    _refused(call(im, o, 8, rows, gain.ctypes.data), r"slot mask 8 is outside 1 \.\. 7")
    _refused(call(im, o, 7, rows, None), r"gain table is needed")
    _refused(call([im[0], None, im[2]], o, 7, rows, gain.ctypes.data), r"slot 1 are needed")
    _refused(call(im, [o[0], o[1], None], 4, rows, gain.ctypes.data), r"slot 2 are needed")
    _refused(call(im, [o[0] + 2, o[1], o[2]], 1, rows, gain.ctypes.data), r"multiples of 4 bytes")
    _refused(call(im, o, 1, rows, gain.ctypes.data + 1), r"multiples of 4 bytes")
    _refused(call(im, [o[0], o[0] + area - 4, o[2]], 3, rows, gain.ctypes.data), r"intersect")
    _refused(call(im, [im[1], o[1], o[2]], 3, rows, gain.ctypes.data), r"intersect")       # slot 0 written over slot 1's input
    _refused(call([o[0] + 4, im[1], im[2]], o, 1, rows, gain.ctypes.data), r"intersect")    # a shifted overlap is not in place
    assert (big == 0xA5).all() and list(sat) == [7, 7, 7] and all(np.array_equal(a, b) for a, b in zip(pics, U.pictures(rows)))
    # what is not selected is not looked at: a missing, misaligned or overlapping slot that is not selected is fine
    assert call([im[0], 1, None], [o[0], im[0], None], 1, rows, gain.ctypes.data) == 0
    assert (big[area:] == 0xA5).all() and not (big[:area] == 0xA5).all()


def test_nodes_and_host_refusals():
    from meteor_demod_amd import _capi, sun
    from meteor_demod_amd import map as mp
    L = sun.lib()
    tm, tle, mo = U.timing("day", 4), mp.parse_tle(M.tle_text()), mp.make_opts(**U.map_opts("day"))
    gain = np.full((5, 99), 0x5A5A5A5A, np.uint32)

    def nodes(limit=85.0, ref=45.0, rows=4, g=gain.ctypes.data, tle_=tle, mo_=mo):
        return L.mdemod_sun_nodes(C.byref(tle_), C.byref(tm), C.byref(mo_), C.byref(sun.options(limit, ref)), rows, g, None)
    _refused(nodes(limit=59.9), r"limit_deg 59\.9 is outside 60 \.\. 89")
    _refused(nodes(limit=89.1), r"limit_deg 89\.1 is outside 60 \.\. 89")
    _refused(nodes(limit=float("nan")), r"limit_deg nan is outside")
    _refused(nodes(ref=-0.5), r"ref_deg -0\.5 is outside 0 \.\. 80")
    _refused(nodes(ref=80.5), r"ref_deg 80\.5 is outside 0 \.\. 80")
    _refused(nodes(rows=0), r"0 strip rows")
    _refused(nodes(rows=8193), r"8193 strip rows")
    _refused(nodes(g=None), r"gain table is needed")
    bad_tle = mp.parse_tle(M.tle_text())
    bad_tle.inclination_deg = 200.0
    _refused(nodes(tle_=bad_tle), r"inclination")
    bad_mo = mp.make_opts(**U.map_opts("day"))
    bad_mo.scan_deg = 131.0
    _refused(nodes(mo_=bad_mo), r"scan")
    assert (gain == 0x5A5A5A5A).all()
    assert nodes() == 0 and (gain != 0x5A5A5A5A).all()
    _refused(L.mdemod_sun_position(20000, float("inf"), C.byref((C.c_double * 3)())), r"no time of day")
    _refused(L.mdemod_sun_position(20000, 0.0, None), r"vector is needed")
    # the host entry (the model's, which needs no device): no placed packet, a missing picture of a reflective slot, options
    pics = U.pictures(4)
    place, info = U.packets("day", 4)
    with pytest.raises(_capi.MdemodError, match="no placed packet"):
        sun.correct_images(pics, (64, 65, 66), place[:0], info[:0], M.tle_text(), model=True, **U.map_opts("day"))
    with pytest.raises(_capi.MdemodError, match=r"limit_deg 90 is outside"):
        sun.correct_images(pics, (64, 65, 66), place, info, M.tle_text(), model=True, limit_deg=90, **U.map_opts("day"))
    with pytest.raises(TypeError, match="no option"):
        sun.correct_images(pics, (64, 65, 66), place, info, M.tle_text(), model=True, limit=80)
    pi, ids, summ = (C.c_void_p * 3)(pics[0].ctypes.data, None, pics[2].ctypes.data), (C.c_uint32 * 3)(64, 65, 68), sun.Summary()
    _refused(L.mdemod_sun_model_host(None, C.byref(mo), C.byref(tle), C.byref(pi), C.byref(ids), 4, place.ctypes.data, info.ctypes.data, place.size, C.byref(summ)),
             r"slot 1 \(APID 65\) is needed")
    assert all(np.array_equal(a, b) for a, b in zip(pics, U.pictures(4)))


def test_defaults_workspace_and_bindings():
    from meteor_demod_amd import sun
    o = sun.default_opts()
    assert (o.limit_deg, o.ref_deg, list(o.reserved)) == (85.0, 45.0, [0, 0, 0, 0])
    assert [sun.workspace(r) for r in (0, 1, 77, 8192, 8193)] == [0, 12, 924, 98304, 0]
    header = (ROOT / "include" / "meteor_demod_amd_sun.h").read_text()
    declared = set(re.findall(r"\b(mdemod_sun_\w+)\s*\(", header.split("#ifndef")[1]))
    print(sorted(declared))
    assert declared == set(sun.SIGNATURES) and all(hasattr(sun.lib(), n) for n in list(sun.SIGNATURES) + list(sun.MODEL_SIGNATURES))
    assert C.sizeof(sun.Opts) == 32 and C.sizeof(sun.Summary) == 64
    for word in ("to be confirmed off air", "dark level", "45 degrees", "64 .. 66"):
        assert word in header


# ------------------------------------------------------------------------------------------------------------------ slot rule
def test_a_thermal_channel_stays_as_decoded():
    from meteor_demod_amd import sun
    rows = 6
    pics = U.pictures(rows)
    place, info = U.packets("terminator", rows)
    opts = U.map_opts("terminator")
    gain = U.gain_table("terminator", rows)
    out, summ = sun.correct_images(pics, (64, 68, 66), place, info, M.tle_text(), model=True, **opts)
    want, sat = S.apply(pics, gain, 5)
    lib_gain, _ = sun.nodes(M.tle_text(), U.timing("terminator", rows), rows, **opts)
    want_lib, sat_lib = sun.model_apply(pics, lib_gain, 5)
    print(f"APIDs 64, 68, 66: mask {summ['slot_mask']}, saturated {summ['saturated']} (sun_ref on its own nodes {sat}); zenith {summ['zenith_min']:.2f} .. {summ['zenith_max']:.2f}")
    assert summ["slot_mask"] == 5 and summ["saturated"] == sat_lib and summ["saturated"][1] == 0
    assert np.array_equal(out[1], pics[1])                                          # byte for byte
    assert all(np.array_equal(out[k], want_lib[k]) and not np.array_equal(out[k], pics[k]) for k in (0, 2))
    # sun_ref's own nodes differ from the library's by rounding ties at most: so do the pictures, by one level at a few pixels
    if np.array_equal(lib_gain, gain):
        assert all(np.array_equal(out[k], want[k]) for k in (0, 2)) and summ["saturated"] == sat
    # nothing reflective: nothing happens
    out, summ = sun.correct_images(pics, (67, 68, 69), place, info, M.tle_text(), model=True, **opts)
    assert summ["slot_mask"] == 0 and all(np.array_equal(a, b) for a, b in zip(out, pics)) and summ["nodes"] == (rows + 1) * 99
