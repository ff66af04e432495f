"""CPU tests of the equalise layer (include/meteor_demod_amd_equalise.h): the C++ host model against the numpy model of
tests/equalise_ref.py, byte for byte, over the sizes, pictures and masks both suites use; the redistribution on 10^4 histograms; the
tables' shape; amount 0; uncounted pixels; one tile without a clip against plain histogram equalisation; every refusal; the defaults
and the workspace; the binding tables; and the C host's refusals, which need no GPU.  Every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import equalise_ref as R
from conftest import ROOT

CLIPS = (100, 300, 25600)
AMOUNTS = (0, 128, 256)


def _cases(size):
    """Every picture, mask and layout at one size; the clips and amounts go round so that each pair meets each of them."""
    w, h, tile = size
    i = 0
    for kind in R.PICTURES:
        for mask in R.MASKS:
            for planes, mode in R.LAYOUTS:
                yield kind, mask, planes, mode, CLIPS[i % 3], AMOUNTS[(i // 3 + i) % 3]
                i += 1


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}t{s[2]}")
def test_model_equals_numpy_model(size):
    from meteor_demod_amd import equalise as E
    w, h, tile = size
    n = empty = changed = 0
    for kind, mask, planes, mode, clip, amount in _cases(size):
        pic = R.picture_of(kind, w, h, planes)
        valid, step = R.mask_of(mask, kind, w, h, tile)
        kw = dict(tile=tile, clip=clip / 100.0, amount=amount / 256.0, mode=mode, valid_step=step)
        tab, count = E.model_tables(pic, valid, **kw)
        out = E.model_apply(pic, valid, **kw)
        want, rtab, rcount = R.equalise(pic, valid, tile, clip, amount, mode, step)
        what = (size, kind, mask, planes, mode, clip, amount)
        assert tab.shape == rtab.shape and np.array_equal(count, rcount), what
        assert np.array_equal(tab, rtab), what
        assert np.array_equal(out, want), what
        # every table of a tile that is not empty is non-decreasing and ends at 255; an empty tile's is 256 zeroes
        full = count != 0
        assert (np.diff(tab[full].astype(int), axis=-1) >= 0).all() and (tab[full][..., 255] == 255).all() and not tab[~full].any(), what
        if mask == "nothing":
            assert not count.any() and np.array_equal(out, pic), what
        n += 1
        empty += int((count == 0).sum())
        changed += int((out != pic).sum())
    print(f"{size}: {n} cases, {empty} empty tiles, {changed} bytes changed")
    assert n == 75 and empty > 0
    assert changed > 0


def _histograms():
    rng = np.random.default_rng(5)
    spike = np.zeros(256, np.uint32); spike[200] = 767 * 767
    one = np.zeros(256, np.uint32); one[0] = 1
    last = np.zeros(256, np.uint32); last[255] = 1
    full = np.full(256, 767 * 767 // 256, np.uint32); full[:767 * 767 % 256] += 1
    out = [spike, one, last, full, np.full(256, 9, np.uint32), np.zeros(256, np.uint32)]
    while len(out) < 10000:
        k = len(out) % 4
        if k == 0:
            h = rng.integers(0, 2300, 256)
        elif k == 1:
            h = np.bincount(rng.integers(0, 256, int(rng.integers(1, 3000))), minlength=256)
        elif k == 2:
            h = np.zeros(256, np.int64); h[rng.integers(0, 256, int(rng.integers(1, 6)))] = rng.integers(1, 100000)
        else:
            h = (rng.integers(0, 40, 256) ** 2) * (rng.integers(0, 3, 256) == 0)
        out.append(h.astype(np.uint32))
    assert int(full.sum()) == 767 * 767
    return out


def test_redistribution_keeps_the_count_and_tables_rise_to_255():
    from meteor_demod_amd import equalise as E
    rng = np.random.default_rng(6)
    seen_n, clipped = set(), 0
    for k, hist in enumerate(_histograms()):
        clip = (100, 300, 25600, int(rng.integers(100, 25601)))[k % 4]
        n, h2, tab = E.model_table(hist, clip)
        rh2, rtab = R.table_of(hist, clip)
        assert n == int(hist.sum()) and int(h2.sum(dtype=np.int64)) == n, (k, clip)
        assert np.array_equal(h2, rh2) and np.array_equal(tab, rtab), (k, clip)
        if n:
            assert (np.diff(tab.astype(int)) >= 0).all() and tab[255] == 255, (k, clip)
            clipped += int((h2 != hist).any())
        else:
            assert not tab.any()
        if clip == 25600:
            assert np.array_equal(h2, hist)
        seen_n.add(n)
    print(f"10000 histograms, {len(seen_n)} different n, {clipped} clipped; n = 1 and n = 767^2 among them: {1 in seen_n}, {767 * 767 in seen_n}")
    # (a quarter of the draws has clip 100, L = ceil(n / 256), where every histogram that is not flat is clipped)
    assert {0, 1, 767 * 767} <= seen_n and clipped > 2000


def test_amount_zero_is_the_identity_and_uncounted_pixels_stay():
    from meteor_demod_amd import equalise as E
    for planes, mode in R.LAYOUTS:
        pic = R.picture_of("noise", 75, 50, planes)
        valid, _ = R.mask_of("half", "noise", 75, 50, 16)
        # luminance mode at amount 0: out = (c Y + Y / 2) / Y = c
        out0 = E.model_apply(pic, valid, tile=16, clip=3.0, amount=0.0, mode=mode)
        out1 = E.model_apply(pic, valid, tile=16, clip=3.0, amount=1.0, mode=mode)
        keep = valid == 0
        print(f"planes {planes} mode {mode}: amount 0 changes {int((out0 != pic).sum())} bytes, amount 1 changes {int((out1 != pic).sum())}, "
              f"{int((out1[keep] != pic[keep]).sum())} of them uncounted")
        assert np.array_equal(out0, pic)
        assert np.array_equal(out1[keep], pic[keep]) and (out1[~keep] != pic[~keep]).any()


def test_one_tile_without_clip_is_plain_histogram_equalisation():
    from meteor_demod_amd import equalise as E
    rng = np.random.default_rng(8)
    pic = (rng.normal(90, 20, (20, 19)).clip(0, 255)).astype(np.uint8)
    tab, count = E.model_tables(pic, None, tile=16, clip=256.0)
    out = E.model_apply(pic, None, tile=16, clip=256.0)
    n = pic.size
    cum = np.cumsum(np.bincount(pic.ravel(), minlength=256))
    want = ((255 * cum + n // 2) // n).astype(np.uint8)
    print(f"one tile of {n} pixels: table from {want[0]} to {want[255]}, {len(np.unique(out))} levels out")
    assert tab.shape == (1, 1, 1, 256) and count[0, 0, 0] == n
    assert np.array_equal(tab[0, 0, 0], want) and np.array_equal(out, want[pic])


def test_defaults_and_workspace():
    from meteor_demod_amd import equalise as E
    o = E.default_opts()
    assert (o.tile, o.clip_percent, o.amount, o.mode, o.valid_step, list(o.reserved)) == (128, 300, 256, 1, 1, [0, 0, 0])
    assert C.sizeof(E.Opts) == 32 and C.sizeof(E.Summary) == 16
    for (w, h, planes, tile, mode) in ((1, 1, 1, 16, 1), (2784, 1440, 3, 128, 1), (2784, 1440, 3, 128, 0), (8192, 16384, 3, 16, 0), (8192, 16384, 1, 512, 1), (767, 767, 3, 512, 0),
                                       (39, 23, 1, 16, 1), (40, 24, 1, 16, 1)):
        nx, ny = max(1, (w + tile // 2) // tile), max(1, (h + tile // 2) // tile)
        ch = 3 if planes == 3 and mode == 0 else 1
        got = E.workspace(w, h, planes, E.options(tile=tile, mode=mode))
        print(f"{w} x {h} x {planes} tile {tile} mode {mode}: {nx} x {ny} tiles, {ch} channels, {got} bytes")
        assert got == ch * ny * nx * (256 + 4) and E.geometry(w, h, planes, E.options(tile=tile, mode=mode)) == (ch, ny, nx)
    assert E.workspace(2784, 1440, 3) == 22 * 11 * 260
    assert E.geometry(39, 23, 1, E.options(tile=16))[1:] == (1, 2) and E.geometry(40, 24, 1, E.options(tile=16))[1:] == (2, 3)
    for bad in ((0, 5, 1, {}), (8193, 5, 1, {}), (5, 0, 1, {}), (5, 16385, 1, {}), (5, 5, 2, {}), (5, 5, 1, dict(tile=8)), (5, 5, 1, dict(tile=20)), (5, 5, 1, dict(tile=520)),
                (5, 5, 1, dict(clip=0.99)), (5, 5, 1, dict(clip=256.01)), (5, 5, 1, dict(amount=1.01)), (5, 5, 3, dict(mode=2)), (5, 5, 1, dict(valid_step=2))):
        assert E.workspace(*bad[:3], E.options(**bad[3])) == 0, bad
    assert E.workspace(5, 5, 1, E.options(mode=2)) == 260                        # mode is ignored for planes 1


def test_model_refusals():
    from meteor_demod_amd import _capi, equalise as E
    pic = R.picture_of("noise", 40, 24, 3)
    lib = E.lib()
    for word, kw in (("tile", dict(tile=8)), ("tile", dict(tile=100)), ("tile", dict(tile=1024)), ("clip_percent", dict(clip=0.5)), ("clip_percent", dict(clip=300.0)),
                     ("amount", dict(amount=2.0)), ("mode", dict(mode=2)), ("valid_step", dict(valid_step=4))):
        for call in (E.model_tables, E.model_apply):
            with pytest.raises(_capi.MdemodError) as e:
                call(pic, None, **kw)
            print(e.value.detail)
            assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail
    o = E.options(tile=16)
    need = E.workspace(40, 24, 3, o)
    work = np.zeros(need + 64, np.uint8)
    out = np.full(pic.size + 8, 0xA5, np.uint8)
    P, Wk, O = pic.ctypes.data, work.ctypes.data, out.ctypes.data

    def refused(word, rc):
        assert rc == _capi.MDEMOD_ERR_PARAM and word in _capi.last_error(), (word, rc, _capi.last_error())
        print(_capi.last_error())
    refused("width", lib.mdemod_equalise_model_tables(P, None, 0, 24, 3, C.byref(o), Wk, need))
    refused("height", lib.mdemod_equalise_model_tables(P, None, 40, 16385, 3, C.byref(o), Wk, need))
    refused("planes", lib.mdemod_equalise_model_tables(P, None, 40, 24, 2, C.byref(o), Wk, need))
    refused("picture is needed", lib.mdemod_equalise_model_tables(None, None, 40, 24, 3, C.byref(o), Wk, need))
    refused("workspace is needed", lib.mdemod_equalise_model_tables(P, None, 40, 24, 3, C.byref(o), None, need))
    refused(f"needs {need} bytes", lib.mdemod_equalise_model_tables(P, None, 40, 24, 3, C.byref(o), Wk, need - 1))
    refused("multiples of 4", lib.mdemod_equalise_model_tables(P, None, 40, 24, 3, C.byref(o), Wk + 2, need))
    refused("multiples of 4", lib.mdemod_equalise_model_tables(P + 1, None, 40, 23, 3, C.byref(o), Wk, need))
    refused("intersect", lib.mdemod_equalise_model_tables(P, None, 40, 24, 3, C.byref(o), P + 2000, need))
    refused("intersect", lib.mdemod_equalise_model_tables(P, P + 40, 40, 23, 3, C.byref(o), Wk, need))
    assert not work.any()
    assert lib.mdemod_equalise_model_tables(P, None, 40, 24, 3, C.byref(o), Wk, need) == 0
    refused("output is needed", lib.mdemod_equalise_model_apply(P, None, 40, 24, 3, C.byref(o), Wk, None))
    refused("multiples of 4", lib.mdemod_equalise_model_apply(P, None, 40, 24, 3, C.byref(o), Wk, O + 1))
    refused("intersect", lib.mdemod_equalise_model_apply(P, None, 40, 24, 3, C.byref(o), Wk, P + 4))
    refused("intersect", lib.mdemod_equalise_model_apply(P, None, 40, 24, 3, C.byref(o), Wk, Wk + 4))
    refused("intersect", lib.mdemod_equalise_model_apply(P, O + 4, 40, 24, 3, C.byref(o), Wk, O))
    assert (out == 0xA5).all()
    # in place is the one exception
    want = E.model_apply(pic, None, tile=16)
    same = pic.copy()
    assert lib.mdemod_equalise_model_apply(same.ctypes.data, None, 40, 24, 3, C.byref(o), Wk, same.ctypes.data) == 0
    assert np.array_equal(same, want) and not np.array_equal(same, pic)
    # no options: the defaults
    assert lib.mdemod_equalise_model_tables(P, None, 40, 24, 3, None, Wk, need) == 0


def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", (ROOT / "include" / "meteor_demod_amd_equalise.h").read_text(), re.M)


def test_equalise_entries_exported_and_bound():
    from meteor_demod_amd import _capi, equalise as E, jpeg
    names = _header_entries()
    print(names)
    assert sorted(names) == sorted(E.SIGNATURES) and len(names) == 6
    lib = E.lib()
    for n in names + list(E.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(E.MODEL_SIGNATURES) == ["mdemod_equalise_model_apply", "mdemod_equalise_model_table", "mdemod_equalise_model_tables"]
    listed = (ROOT / "meteor_demod_amd" / "csrc" / "equalise_host.h").read_text()
    assert all(n in listed for n in E.MODEL_SIGNATURES)
    assert not any("equalise" in n for n in list(_capi.SIGNATURES) + list(jpeg.SIGNATURES) + list(jpeg.MODEL_SIGNATURES))
    for h in (ROOT / "include").glob("*.h"):
        if h.name != "meteor_demod_amd_equalise.h":
            assert "mdemod_equalise_" not in h.read_text(), h.name
    for f in ("apply", "tables", "model_tables", "model_apply", "workspace"):
        assert callable(getattr(E, f))
    # the header's opening comment is the specification the numpy model was written from
    head = (ROOT / "include" / "meteor_demod_amd_equalise.h").read_text().split("*/")[0]
    for word in ("picture", "valid", "channels", "tiles", "histogram", "clip", "table", "workspace", "apply", "amount", "output", "refused"):
        assert re.search(rf"^ \*   {word}\s", head, re.M), word


def test_cli_refusals(tmp_path):
    """What the C host refuses before it opens a file or a device."""
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    (tmp_path / "in.wav").write_bytes(b"")
    derived = ("--image", "--rectify")
    for flags, word in ((("--equalise", "3"), "only with --image"),
                        (("--image", "--equalise", "3"), "only with --rectify, --composite or --map"),
                        ((*derived, "--equalise", "0.5"), "1 .. 256"), ((*derived, "--equalise", "257"), "1 .. 256"), ((*derived, "--equalise", "x"), "1 .. 256"),
                        ((*derived, "--equalise", "3", "--equalise-tile", "100"), "multiple of 8"), ((*derived, "--equalise", "3", "--equalise-tile", "8"), "16 .. 512"),
                        ((*derived, "--equalise", "3", "--equalise-tile", "520"), "16 .. 512"), ((*derived, "--equalise", "3", "--equalise-amount", "101"), "0 .. 100"),
                        ((*derived, "--equalise", "3", "--equalise-amount", "-1"), "0 .. 100"),
                        ((*derived, "--equalise-tile", "64"), "only with --equalise"), ((*derived, "--equalise-amount", "50"), "only with --equalise")):
        r = subprocess.run([str(cli_exe), "-q", "-B", *flags, "-o", "no.s", "in.wav"], capture_output=True, text=True, cwd=tmp_path, timeout=60)
        print(flags, "->", r.returncode, r.stderr.strip())
        assert r.returncode == 1 and word in r.stderr and not (tmp_path / "no.s").exists(), (flags, r.stderr)
    h = subprocess.run([str(cli_exe), "--help"], capture_output=True, text=True, timeout=60)
    text = h.stdout + h.stderr
    assert all(w in text for w in ("--equalise <clip>", "--equalise-tile <pixels>", "--equalise-amount <percent>"))
