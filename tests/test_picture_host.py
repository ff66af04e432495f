"""CPU tests of the picture layer (include/meteor_demod_amd_picture.h): the column map's symmetry, range, width and centre, the map
against picture_util's float64 restatement, the identity map, the refusals, the contrast table on the cases that take a different
branch each, the render model against the utility byte for byte, the pieces of the whole-picture entry's model path, and the
binding table.  Every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import picture_util as PU
from conftest import ROOT

HEADER = ROOT / "include" / "meteor_demod_amd_picture.h"
TOP = 1567 * 256


@pytest.fixture(scope="module")
def picture():
    from meteor_demod_amd import picture as m
    return m


# ---------------------------------------------------------------------------------------------------------------- the map
@pytest.mark.parametrize("opts", PU.OPTION_SETS, ids=["default", "600-100", "900-114", "820-20"])
def test_map_symmetry_range_width_centre_and_numpy(picture, opts):
    m = picture.column_map(**opts).astype(np.int64)
    w = m.size
    want = PU.column_map(**opts).astype(np.int64)
    step = np.diff(m)
    worst = int(np.abs(m - want).max()) if want.size == w else -1
    print(f"{opts or 'defaults'}: W {w} (numpy {want.size}), map[0] {m[0]}, smallest step {step.min()}, centre step {step[w // 2 - 1]}, "
          f"largest difference from numpy {worst} / 256 pixel")
    assert w % 4 == 0 and w == want.size
    assert np.array_equal(m + m[::-1], np.full(w, TOP))                            # symmetric
    assert (step >= 0).all() and m.min() >= 0 and m.max() <= TOP                   # non-decreasing, inside the source line
    assert PU.source_x(w, **opts)[0] >= 0.0 and PU.source_x(w + 4, **opts)[0] < 0.0   # W is maximal
    assert abs(int(step[w // 2 - 1]) - 256) <= 1
    assert worst <= 1                                                             # a last-bit difference between two libms, no more


def test_identity_map(picture):
    m = picture.column_map(rectify=0)
    assert m.dtype == np.uint32 and np.array_equal(m, 256 * np.arange(1568))
    assert np.array_equal(picture.column_map(rectify=0, altitude_km=500, scan_deg=30), m)


def test_map_room_and_width_query(picture):
    from meteor_demod_amd import _capi
    o = picture.make_opts()
    w = C.c_uint32(0)
    assert picture.lib().mdemod_picture_column_map(C.byref(o), None, 0, C.byref(w)) == 0 and w.value == 2784
    few = np.full(2784, 0xAAAAAAAA, dtype=np.uint32)
    assert picture.lib().mdemod_picture_column_map(C.byref(o), few.ctypes.data, 2780, C.byref(w)) == _capi.MDEMOD_ERR_PARAM
    assert "room" in _capi.last_error() and w.value == 2784 and (few == 0xAAAAAAAA).all()
    assert picture.lib().mdemod_picture_column_map(None, None, 0, None) == _capi.MDEMOD_ERR_PARAM and "width" in _capi.last_error()


@pytest.mark.parametrize("word,opts", [("altitude", dict(altitude_km=299.9)), ("altitude", dict(altitude_km=2000.1)), ("altitude", dict(altitude_km=float("nan"))),
                                       ("scan angle", dict(scan_deg=0.9)), ("scan angle", dict(scan_deg=130.1)),
                                       ("misses the Earth", dict(altitude_km=2000.0, scan_deg=100.0)), ("clips", dict(clip_low=500)),
                                       ("clips", dict(clip_high=500)), ("piece_rows", dict(piece_rows=65537))])
def test_refusals(picture, word, opts):
    from meteor_demod_amd import _capi
    with pytest.raises(_capi.MdemodError) as e:
        picture.column_map(**opts)
    print(f"{opts}: '{e.value.detail}'")
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    images, filled = PU.pixels(1, 0), PU.masks("all", 1)
    with pytest.raises(_capi.MdemodError) as e:
        picture.model_host(images, filled, (0, 1, 2), **opts)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail


def test_model_argument_refusals(picture):
    from meteor_demod_amd import _capi
    images, filled = PU.pixels(1, 0), PU.masks("all", 1)
    cmap, luts = picture.column_map(rectify=0), PU.random_luts()
    for word, call in (("planes", lambda: picture.model_host(images, filled, (0, 1))), ("slot", lambda: picture.model_host(images, filled, (0, 1, 3))),
                       ("slot 1", lambda: picture.model_host([images[0], None, images[2]], filled, (0, 1, 2))),
                       ("width", lambda: picture.model_render(images, filled, (0,), luts[:1], cmap[:1566])),
                       ("planes", lambda: picture.model_render(images, filled, (0, 1), luts[:2], cmap))):
        with pytest.raises(_capi.MdemodError) as e:
            call()
        print(f"{word}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        picture.lut(np.ones(256), clip_low=500)
    assert "clips" in e.value.detail


# -------------------------------------------------------------------------------------------------------------- the table
def test_lut_cases(picture):
    ident = np.arange(256, dtype=np.uint8)
    empty = np.zeros(256, np.uint32)
    t, lim = picture.lut(empty, limits=True)
    assert np.array_equal(t, ident) and lim == (0, 255)                           # N = 0
    const = empty.copy(); const[77] = 12544
    t, lim = picture.lut(const, limits=True)
    assert np.array_equal(t, ident) and lim == (0, 255)                           # a constant picture: hi = lo
    # hi < lo cannot come from one histogram with clips below 500 permille; hi == lo is the constant picture above and this one:
    near = empty.copy(); near[10], near[11], near[12] = 1, 998, 1
    t, lim = picture.lut(near, 5, 5, limits=True)
    assert np.array_equal(t, ident) and lim == (0, 255), lim                      # both clips land on the one full bin
    # clips 0 / 0: the limits are the first and the last occupied bin
    few = empty.copy(); few[[20, 100, 220]] = [1, 50, 1]
    t, lim = picture.lut(few, 0, 0, limits=True)
    assert lim == (20, 220) and t[20] == 0 and t[220] == 255 and t[19] == 0 and t[221] == 255 and t[120] == (100 * 255 + 100) // 200
    # the same with the default clips: 1 of 52 pixels is more than 5 permille, nothing is clipped
    assert picture.lut(few, limits=True)[1] == (20, 220)
    # two spikes: everything between them is spread over the whole range
    two = empty.copy(); two[50], two[150] = 1000, 1000
    t, lim = picture.lut(two, limits=True)
    assert lim == (50, 150) and t[50] == 0 and t[150] == 255 and t[100] == (50 * 255 + 50) // 100 and (np.diff(t.astype(int)) >= 0).all()
    print(f"two spikes: limits {lim}, table[100] {t[100]}; clips 0/0: {picture.lut(few, 0, 0, limits=True)[1]}")
    assert np.array_equal(picture.lut(two, stretch=False), ident)
    rng = np.random.default_rng(5)
    for k in range(300):
        h = (rng.integers(0, 1 << int(rng.integers(1, 31)), 256) * (rng.random(256) < rng.random())).astype(np.uint32)
        cl, ch = int(rng.integers(0, 500)), int(rng.integers(0, 500))
        got, lim = picture.lut(h, cl, ch, limits=True)
        want, lo, hi = PU.lut(h, cl, ch)
        assert np.array_equal(got, want) and lim == (lo, hi), (k, cl, ch, lim, (lo, hi))
    # the largest counts a picture can give: 65 536 rows of one value
    big = empty.copy(); big[3], big[200] = 65536 * 8 * 1568 - 1, 1
    got, lim = picture.lut(big, 0, 0, limits=True)
    assert lim == (3, 200) and np.array_equal(got, PU.lut(big, 0, 0)[0])


# ------------------------------------------------------------------------------------------------------- the render model
@pytest.mark.parametrize("kind", ["all", "none", "checker", "empty1", "mixed"])
def test_render_model_equals_the_utility(picture, kind):
    """Both given the library's own map, so that no libm enters: planes 1 and 3, a repeated slot, the default, the narrow and the
    identity map, tables whose 0 and 255 are reachable."""
    rows = 3
    images, filled, luts = PU.pixels(rows, 7), PU.masks(kind, rows, 3), PU.random_luts()
    hist = picture.model_histogram(images, filled)
    assert np.array_equal(hist, PU.histogram(images, filled)) and int(hist.sum()) == sum(int((f != 0).sum()) for f in filled) * 896
    assert not picture.model_histogram([images[0], None, images[2]], filled)[1].any()
    for opts in (dict(), dict(altitude_km=820, scan_deg=20), dict(rectify=0)):
        cmap = picture.column_map(**opts)
        for select in ((2, 1, 0), (1,), (0, 0, 2)):
            got, val = picture.model_render(images, filled, select, luts[: len(select)], cmap, valid=True)
            want, want_val = PU.render(images, filled, select, luts[: len(select)], cmap)
            print(f"{kind}, {opts}, select {select}: W {cmap.size}, {np.count_nonzero(val)} of {val.size} columns valid, bytes 0 .. 255: {got.min()} .. {got.max()}")
            assert np.array_equal(got, want) and np.array_equal(val, want_val)
    if kind == "checker":
        one_tap = (val[:, :-1] != 0).sum()
        assert 0 < one_tap < val.size


def test_map_entry_beyond_the_line_reads_the_last_column(picture):
    images, filled = PU.pixels(1, 2), PU.masks("all", 1)
    cmap = np.array([0, TOP, TOP + 255, 0xFFFFFFFF], dtype=np.uint32)
    got = picture.model_render(images, filled, (0,), np.arange(256, dtype=np.uint8)[None], cmap)
    assert np.array_equal(got[:, 1:, 0], np.repeat(images[0][:, 1567:], 3, axis=1)) and np.array_equal(got, PU.render(images, filled, (0,), [np.arange(256)], cmap)[0])


# ----------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("piece", [1, 2, 0])
def test_pieces_equal_one_batch(picture, piece):
    rows = 5
    images, filled = PU.pixels(rows, 11), PU.masks("mixed", rows, 4)
    for select, opts in (((2, 1, 0), dict()), ((1,), dict(scan_deg=20)), ((0, 0, 2), dict(rectify=0, stretch=0)), ((2, 1, 0), dict(clip_low=100, clip_high=0))):
        whole = picture.model_host(images, filled, select, piece_rows=65536, **opts)
        got = picture.model_host(images, filled, select, piece_rows=piece, **opts)
        geo = {k: v for k, v in opts.items() if k in ("altitude_km", "scan_deg", "rectify")}
        want, want_val, lim = PU.compose(images, filled, select, cmap=picture.column_map(**geo), **opts)
        want = want if len(select) == 3 else want[:, :, 0]
        print(f"piece_rows {piece}, select {select}, {opts}: {got.pixels.shape}, limits {got.limits}, {100 * got.valid_share:.1f} % valid")
        assert np.array_equal(got.pixels, whole.pixels) and np.array_equal(got.valid, whole.valid) and got.limits == whole.limits
        assert got.limits == lim and np.array_equal(got.valid, want_val)
        assert np.array_equal(got.pixels, want)
    empty = picture.model_host([np.zeros((0, 1568), np.uint8)] * 3, [np.zeros((0, 14), np.uint8)] * 3, (2, 1, 0), piece_rows=piece)
    assert empty.pixels.shape == (0, 2784, 3) and empty.limits == [(0, 255)] * 3


# ---------------------------------------------------------------------------------------------------------------- binding
def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", HEADER.read_text(), re.M)


def test_picture_entries_exported_and_bound(picture):
    """Every entry of the new header is exported by the library and typed in picture.py's own table; the older binding tables and
    headers are untouched; the model is exported beside them."""
    from meteor_demod_amd import _capi, frames, frontend, image, interleave, rs, survey
    names = _header_entries()
    assert sorted(names) == sorted(["mdemod_picture_default_opts", "mdemod_picture_column_map", "mdemod_picture_histogram_device", "mdemod_picture_lut",
                                    "mdemod_picture_render_device", "mdemod_picture_compose_host", "mdemod_picture_free"])
    lib = picture.lib()
    for n in names + list(picture.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(picture.SIGNATURES) == sorted(names)
    assert sorted(picture.MODEL_SIGNATURES) == ["mdemod_picture_model_histogram", "mdemod_picture_model_host", "mdemod_picture_model_render"]
    others = (list(_capi.SIGNATURES) + list(frontend.SIGNATURES) + list(survey.SIGNATURES) + list(frames.SIGNATURES) + list(frames.MODEL_SIGNATURES) +
              list(rs.SIGNATURES) + list(rs.MODEL_SIGNATURES) + list(interleave.SIGNATURES) + list(image.SIGNATURES) + list(image.MODEL_SIGNATURES))
    assert not any("_picture_" in n for n in others)
    assert all("_picture_" in n for n in list(picture.SIGNATURES) + list(picture.MODEL_SIGNATURES))
    for h in (ROOT / "include").glob("*.h"):
        if h != HEADER:
            assert "mdemod_picture_" not in h.read_text(), h.name
    assert _capi.lib().mdemod_abi_version() == 5
    for f in ("column_map", "histogram", "lut", "render", "compose", "image_to_picture", "model_histogram", "model_render", "model_host"):
        assert callable(getattr(picture, f))


def test_picture_int_entries_are_function_try_blocks(picture):
    found = 0
    entries = set(_header_entries()) | set(picture.MODEL_SIGNATURES)
    for src in (ROOT / "meteor_demod_amd" / "csrc" / "picture.hip", ROOT / "meteor_demod_amd" / "csrc" / "picture_host.cpp"):
        text = src.read_text()
        for m in re.finditer(r"^int\n(mdemod_\w+)\(", text, re.M):
            assert m.group(1) in entries, m.group(1)
            found += 1
            body = text[m.end():]
            assert body[: body.index("{")].rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            assert body[body.index("\n}"):].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 3 + 5, found


def test_picture_struct_layouts(picture, tmp_path):
    import subprocess
    assert C.sizeof(picture.MdemodPictureOpts) == 40 and C.sizeof(picture.MdemodPictureResult) == 64
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_picture.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
           'sizeof(mdemod_picture_opts), sizeof(mdemod_picture_result), offsetof(mdemod_picture_opts, piece_rows), '
           'offsetof(mdemod_picture_result, valid_cells), offsetof(mdemod_picture_result, valid)); return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [40, 64, picture.MdemodPictureOpts.piece_rows.offset, picture.MdemodPictureResult.valid_cells.offset, picture.MdemodPictureResult.valid.offset]
