"""GPU tests of the overlay layer (include/meteor_demod_amd_overlay.h): the draw kernel against the host model over every piece, byte
for byte, picture and mask, on seeded polylines from 4 x 1 to 8192 x 32, grey and colour; a tile of 0 .. 600 pieces (the ends of the
chunk loop); the corner of a wide cap beside a tile; four styles over each other; inside_only under a checkered valid; tiles without
items; canaries around every buffer; the device entry's argument checks; the whole-picture entry in bands; a map of the synthetic
pass; the C host's --overlay and --graticule on maps and a mosaic.  Every GPU step runs once; every test prints the figures it asserts
on."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import map_util as MU
import picture_util as PU
from test_gpu_map import _dev, _pnm, _stream_handle

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (100, 36), (36, 100), (4, 1), (8192, 32))


def _points(O, lines):
    xs = [np.asarray(a, dtype=np.int64) for a, _ in lines]
    first = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).astype(np.uint32)
    return O.Points(np.concatenate(xs).astype(np.int32), np.concatenate([np.asarray(b, dtype=np.int64) for _, b in lines]).astype(np.int32), first)


def _scene(O, w, h, seed, styles):
    """Pieces of seeded polylines for every style: short ones near the picture, one right across it, one far longer than it."""
    rng = np.random.default_rng(seed)
    parts = []
    for s, st in enumerate(styles):
        lines = []
        for _ in range(3 + w // 512):
            n = int(rng.integers(2, 6))
            x0, y0 = int(rng.integers(0, 256 * w)), int(rng.integers(0, 256 * h))
            lines.append((x0 + np.cumsum(rng.integers(-6000, 6000, n)), y0 + np.cumsum(rng.integers(-6000, 6000, n))))
        lines.append(([-3000, 256 * w + 3000], [int(rng.integers(0, 256 * h + 1)), int(rng.integers(0, 256 * h + 1))]))
        lines.append(([128 * w - 100_000_000, 128 * w + 100_000_000], [128 * h - 70_000_000 - 4000 * s, 128 * h + 70_000_000 - 4000 * s]))
        parts.append(O.pieces(_points(O, lines), s, st.half_width, w, h))
    return np.concatenate(parts)


def _gpu(O, pixels, pcs, styles, gpu_device, valid=None):
    w, h = pixels.shape[1], pixels.shape[0]
    tile_first, items = O.bins(pcs, styles, w, h)
    d = _dev(pixels, gpu_device)
    mask = O.draw_pieces(d, pcs, tile_first, items, styles, valid=None if valid is None else _dev(valid, gpu_device), mask=True)
    return d.cpu().numpy(), mask.cpu().numpy(), tile_first


# ------------------------------------------------------------------------------------------------------ kernel against model
@pytest.mark.parametrize("w,h", SIZES)
def test_draw_equals_the_model(w, h, gpu_device):
    from meteor_demod_amd import overlay as O
    styles = [O.Style(128, 256, (255, 255, 0)), O.Style(300, 160, (20, 200, 90)), O.Style(0, 256, (1, 2, 3))]
    rng = np.random.default_rng(w + h)
    for planes in (1, 3):
        pixels = rng.integers(0, 256, (h, w, 3) if planes == 3 else (h, w), dtype=np.uint8)
        pcs = _scene(O, w, h, 7 * w + planes, styles)
        want, want_mask = O.model_pieces(pixels, pcs, styles)
        got, got_mask, tile_first = _gpu(O, pixels, pcs, styles, gpu_device)
        bad = int((got != want).sum()) + int((got_mask != want_mask).sum())
        print(f"{w} x {h} x {planes}: {len(pcs)} pieces, at most {int(np.diff(tile_first.astype(np.int64)).max())} in a tile, {int((want_mask != 0).sum())} pixels drawn, {bad} bytes differ")
        assert bad == 0 and want_mask.any()
        # without the mask: the same picture
        d = _dev(pixels, gpu_device)
        tf, it = O.bins(pcs, styles, w, h)
        assert O.draw_pieces(d, pcs, tf, it, styles) is None and np.array_equal(d.cpu().numpy(), want)


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 600])
def test_one_tile_of_many_pieces(count, gpu_device):
    """The ends of the chunk loop: one tile carrying 0, 1, 255, 256, 257 and 600 pieces of two styles."""
    from meteor_demod_amd import overlay as O
    styles = [O.Style(40, 256, (250, 10, 10)), O.Style(128, 100, (10, 10, 250))]
    rng = np.random.default_rng(count)
    lines = [[], []]
    for k in range(count):
        x0, y0 = int(rng.integers(0, 256 * 32)), int(rng.integers(0, 256 * 32))
        lines[k % 2].append(([x0, x0 + int(rng.integers(-900, 900)) or 5], [y0, y0 + int(rng.integers(-900, 900))]))
    parts = [O.pieces(_points(O, mine), s, styles[s].half_width, 32, 32) for s, mine in enumerate(lines) if mine]
    pcs = np.concatenate(parts) if parts else np.zeros(0, dtype=O.PIECE)
    assert len(pcs) == count
    for planes in (1, 3):
        pixels = rng.integers(0, 256, (32, 32, 3) if planes == 3 else (32, 32), dtype=np.uint8)
        want, want_mask = O.model_pieces(pixels, pcs, styles)
        got, got_mask, tile_first = _gpu(O, pixels, pcs, styles, gpu_device)
        print(f"{count} pieces, {planes} planes: {int(tile_first[1])} items, {int((want_mask != 0).sum())} pixels drawn")
        assert int(tile_first[1]) == count and np.array_equal(got, want) and np.array_equal(got_mask, want_mask)


def test_corner_of_a_wide_cap(gpu_device):
    """The reach trap: a 45 degree piece of the widest style ends 2600 units left of a tile, farther than w + 128 = 2176, in one of
    the tile's rows, and colours pixels of that tile."""
    from meteor_demod_amd import overlay as O
    w, h, half = 96, 96, 2048
    styles = [O.Style(half, 256, (255, 0, 0))]
    end_x, end_y = 256 * 32 - 2600, 256 * 40
    pcs = O.pieces(_points(O, [([end_x - 4000, end_x], [end_y - 4000, end_y])]), 0, half, w, h)
    for pixels in (np.full((h, w, 3), 17, dtype=np.uint8), np.full((h, w), 99, dtype=np.uint8)):
        want, want_mask = O.model_pieces(pixels, pcs, styles)
        got, got_mask, _ = _gpu(O, pixels, pcs, styles, gpu_device)
        print(f"{int(want_mask[32:64, 32:64].sum())} pixels of tile (1, 1) drawn")
        assert want_mask[32:64, 32:64].any() and np.array_equal(got, want) and np.array_equal(got_mask, want_mask)


def test_four_styles_inside_only_and_idle_tiles(gpu_device):
    """Four styles over each other, two of them inside_only under a checkered valid; the tiles without items keep the pattern the
    picture was filled with, byte for byte, and their mask is clear."""
    from meteor_demod_amd import overlay as O
    w, h = 160, 128
    styles = [O.Style(600, 256, (255, 255, 0)), O.Style(300, 128, (0, 255, 255), True), O.Style(128, 200, (255, 0, 255)), O.Style(60, 256, (5, 5, 5), True)]
    # one line that all four share and one of each style's own, all within the tiles (0 .. 1, 0 .. 1)
    pcs = np.concatenate([O.pieces(_points(O, [([2000, 14000], [3000, 9000]), ([9000 - 2000 * s, 3000 + 2000 * s], [1000, 14000])]), s, styles[s].half_width, w, h)
                          for s in range(4)])
    i, j = np.mgrid[0:h, 0:w]
    valid = (((i // 3 + j // 5) % 2) * 9).astype(np.uint8)
    for planes in (1, 3):
        pixels = ((3 * i + 7 * j) % 251).astype(np.uint8) if planes == 1 else np.stack([(3 * i + 7 * j + 50 * p) % 251 for p in range(3)], axis=2).astype(np.uint8)
        want, want_mask = O.model_pieces(pixels, pcs, styles, valid)
        got, got_mask, tile_first = _gpu(O, pixels, pcs, styles, gpu_device, valid)
        idle = np.diff(tile_first.astype(np.int64)).reshape(4, 5) == 0
        seen = sorted(int(v) for v in np.unique(want_mask))
        print(f"{planes} planes: {int(idle.sum())} of 20 tiles without items; mask values {seen}")
        assert np.array_equal(got, want) and np.array_equal(got_mask, want_mask)
        assert 15 in seen and 5 in seen and not (want_mask[valid == 0] & 10).any()
        assert idle.sum() >= 12
        for ty, tx in zip(*np.nonzero(idle)):
            box = (slice(32 * ty, 32 * ty + 32), slice(32 * tx, 32 * tx + 32))
            assert np.array_equal(got[box], pixels[box]) and not got_mask[box].any()


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """The picture, valid and mask at offsets 0, 4 and 1000 inside larger buffers of canaries: the canaries survive, valid is only
    read, and the result is the model's."""
    import torch
    from meteor_demod_amd import overlay as O
    w, h = 100, 70
    styles = [O.Style(200, 256, (255, 255, 0), True), O.Style(128, 160, (128, 128, 128))]
    pcs = _scene(O, w, h, 31 + shift, styles)
    tile_first, items = O.bins(pcs, styles, w, h)
    rng = np.random.default_rng(shift)
    pad = 64 + shift
    for planes in (1, 3):
        pixels = rng.integers(0, 256, (h, w, planes), dtype=np.uint8)
        valid = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        want, want_mask = O.model_pieces(pixels if planes == 3 else pixels[:, :, 0], pcs, styles, valid)
        buf = torch.full((pad + h * w * planes + 64,), 0x5A, dtype=torch.uint8, device=f"cuda:{gpu_device}")
        val = torch.full((pad + h * w + 64,), 0xC3, dtype=torch.uint8, device=f"cuda:{gpu_device}")
        msk = torch.full((pad + h * w + 64,), 0x3C, dtype=torch.uint8, device=f"cuda:{gpu_device}")
        buf[pad: pad + h * w * planes] = _dev(pixels.reshape(-1), gpu_device)
        val[pad: pad + h * w] = _dev(valid.reshape(-1), gpu_device)
        d_pcs, d_first, d_items = _dev(pcs.view(np.uint8), gpu_device), _dev(tile_first.view(np.uint8), gpu_device), _dev(items.view(np.uint8), gpu_device)
        before = val.cpu().numpy()
        assert O.lib().mdemod_overlay_draw_device(C.c_void_p(d_pcs.data_ptr()), len(pcs), C.c_void_p(d_first.data_ptr()), C.c_void_p(d_items.data_ptr()), items.size,
                                                  O._styles(styles), 2, w, h, planes, C.c_void_p(buf.data_ptr() + pad), C.c_void_p(val.data_ptr() + pad),
                                                  C.c_void_p(msk.data_ptr() + pad), gpu_device, _stream_handle(gpu_device)) == 0
        o, m = buf.cpu().numpy(), msk.cpu().numpy()
        print(f"shift {shift}, {planes} planes: canaries of {pad} and 64 bytes around {o.size - pad - 64} and {m.size - pad - 64} bytes")
        for x, canary in ((o, 0x5A), (m, 0x3C)):
            assert (x[:pad] == canary).all() and (x[-64:] == canary).all()
        assert np.array_equal(val.cpu().numpy(), before)
        assert np.array_equal(o[pad:-64].reshape(want.shape), want) and np.array_equal(m[pad:-64].reshape(h, w), want_mask) and want_mask.any()
        assert np.array_equal(d_pcs.cpu().numpy(), pcs.view(np.uint8)) and np.array_equal(d_items.cpu().numpy(), items.view(np.uint8))


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    """Every refusal with its text, and nothing written; no pieces and height 0 draw nothing; two runs on the same input give the
    same bytes."""
    import torch
    from meteor_demod_amd import _capi, overlay as O
    lib, st = O.lib(), _stream_handle(gpu_device)
    w, h = 100, 70
    styles = [O.Style(200, 256, (255, 255, 0)), O.Style(128, 160, (128, 128, 128))]
    pcs = _scene(O, w, h, 5, styles)
    tile_first, items = O.bins(pcs, styles, w, h)
    n_p, n_f, n_i, area = pcs.size * 32, tile_first.size * 4, items.size * 4, w * h
    buf = torch.zeros(n_p + n_f + n_i + 5 * area + 64, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    a_p, a_f, a_i = base, base + n_p, base + n_p + n_f
    a_px, a_val, a_msk = a_i + n_i, a_i + n_i + 3 * area, a_i + n_i + 4 * area
    buf[:n_p] = _dev(pcs.view(np.uint8), gpu_device)
    buf[n_p: n_p + n_f] = _dev(tile_first.view(np.uint8), gpu_device)
    buf[n_p + n_f: n_p + n_f + n_i] = _dev(items.view(np.uint8), gpu_device)
    rng = np.random.default_rng(1)
    pixels, valid = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.integers(0, 2, (h, w)) * 3).astype(np.uint8)
    o = a_px - base

    def fill():
        buf[o: o + 3 * area] = _dev(pixels.reshape(-1), gpu_device)
        buf[o + 3 * area: o + 4 * area] = _dev(valid.reshape(-1), gpu_device)
        buf[o + 4 * area: o + 5 * area] = 0xEE

    def draw(p=a_p, n_pieces=len(pcs), f=a_f, i=a_i, n_items=items.size, sty=styles, n_styles=None, width=w, height=h, planes=3, px=a_px, val=a_val, msk=a_msk):
        return lib.mdemod_overlay_draw_device(C.c_void_p(p), n_pieces, C.c_void_p(f), C.c_void_p(i), n_items, O._styles(sty) if sty is not None else None,
                                              len(sty) if n_styles is None else n_styles, width, height, planes, C.c_void_p(px), C.c_void_p(val), C.c_void_p(msk), gpu_device, st)
    fill()
    assert draw() == 0
    first = buf.cpu().numpy()
    want, want_mask = O.model_pieces(pixels, pcs, styles, valid)
    assert np.array_equal(first[o: o + 3 * area].reshape(h, w, 3), want) and np.array_equal(first[o + 4 * area: o + 5 * area].reshape(h, w), want_mask)
    fill()
    assert draw() == 0 and np.array_equal(buf.cpu().numpy(), first)              # two runs: the same bytes
    # nothing to draw: the picture stays and the mask is cleared; height 0 looks at no pointer
    fill()
    assert draw(n_pieces=0, p=0, f=0, i=0, n_items=0) == 0 and draw(height=0, px=0, msk=0) == 0
    now = buf.cpu().numpy()
    assert np.array_equal(now[o: o + 3 * area], pixels.reshape(-1)) and not now[o + 4 * area: o + 5 * area].any()
    fill()
    before = buf.cpu().numpy()
    inside = [O.Style(200, 256, (1, 1, 1), True)]
    for word, change in (("planes", dict(planes=2)), ("styles (1 .. 4)", dict(n_styles=0)), ("styles (1 .. 4)", dict(sty=styles * 3)), ("styles are needed", dict(sty=None, n_styles=1)),
                         ("half width", dict(sty=[O.Style(2049)])), ("opacity", dict(sty=[O.Style(128, 257)])), ("width", dict(width=w - 2)), ("width", dict(width=0)),
                         ("width", dict(width=8196)), ("height", dict(height=16385)), ("picture is needed", dict(px=0)), ("valid is needed", dict(sty=inside, val=0)),
                         ("are needed", dict(p=0)), ("are needed", dict(f=0)), ("are needed", dict(i=0)), ("2^31", dict(n_items=1 << 31)),
                         ("multiples of 4", dict(px=a_px + 2)), ("multiples of 4", dict(val=a_val + 1)), ("multiples of 4", dict(msk=a_msk + 3)),
                         ("multiples of 4", dict(p=a_p + 2)), ("multiples of 4", dict(f=a_f + 1)), ("multiples of 4", dict(i=a_i + 2)),
                         ("intersect", dict(px=a_p + 4)), ("intersect", dict(px=a_f - 3 * area + 4)), ("intersect", dict(px=a_i)), ("intersect", dict(msk=a_px + 4)),
                         ("intersect", dict(msk=a_val)), ("intersect", dict(px=a_val - 3 * area + 4)), ("intersect", dict(msk=a_i + n_i - 4)), ("intersect", dict(val=a_px + 8))):
        rc = draw(**change)
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(buf.cpu().numpy(), before)                               # nothing was written


# ---------------------------------------------------------------------------------------------------------------- bands
def _coast(g, seed):
    from meteor_demod_amd import overlay as O
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(4):
        n = int(rng.integers(3, 30))
        lon = g.lon_left + g.width / g.sx * rng.uniform(0, 1) + np.cumsum(rng.uniform(-1.0, 1.0, n)) * 20 / g.sx
        lat = g.lat_top - g.height / g.sy * rng.uniform(0, 1) + np.cumsum(rng.uniform(-1.0, 1.0, n)) * 20 / g.sy
        lines.append((lon - 360.0 * np.floor((lon + 180.0) / 360.0), np.clip(lat, -90, 90)))
    return O.vectors(lines)


def test_draw_host_in_bands_equals_the_model(gpu_device):
    """mdemod_overlay_draw_host in bands of 32, 64 and 1024 lines: the bytes, the mask and the report of the model's host entry, which
    are those of the model over every piece; ``draw`` on a device tensor gives them too."""
    from meteor_demod_amd import _capi, overlay as O
    g = O.Geo(200, 150, 12, 10.0, 44.0, 170.0)                                     # across the date line
    rng = np.random.default_rng(8)
    layers, styles = [(_coast(g, 3), 0), (O.graticule(g, 2), 1)], O.default_styles(width=2.0)
    styles[1].inside_only = True
    valid = (rng.integers(0, 4, (150, 200)) != 0).astype(np.uint8)
    for planes in (3, 1):
        pixels = rng.integers(0, 256, (150, 200, 3) if planes == 3 else (150, 200), dtype=np.uint8)
        want, want_mask, want_rep = O._host(O.lib().mdemod_overlay_model_host, "model", pixels, g, layers, styles, valid, True, 0, ())
        direct = O.model_pieces(pixels, O.layer_pieces(g, layers, styles), styles, valid)
        assert np.array_equal(direct[0], want) and np.array_equal(direct[1], want_mask)
        for piece in (32, 64, 0):
            got, got_mask, rep = O.draw_host(pixels, g, layers, styles, valid, piece_lines=piece, device=gpu_device)
            assert np.array_equal(got, want) and np.array_equal(got_mask, want_mask) and rep == want_rep, piece
        print(f"{planes} planes: {want_rep}")
        assert min(want_rep.pixels) > 0 and want_rep.tiles > 5
        on_device, device_mask = O.draw(_dev(pixels, gpu_device), g, layers, styles, valid=_dev(valid, gpu_device), mask=True)
        assert np.array_equal(on_device.cpu().numpy(), want) and np.array_equal(device_mask.cpu().numpy(), want_mask)
    with pytest.raises(_capi.MdemodError) as e:
        O.draw_host(pixels, g, layers, styles, valid, piece_lines=48, device=gpu_device)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "piece_lines" in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        O.draw_host(pixels, g, layers, styles, None, device=gpu_device)
    assert "valid is needed" in e.value.detail


def test_draw_map_on_the_synthetic_pass(gpu_device):
    """A map of the synthetic pass of map_util.py with a coast and a graticule: ``draw_map`` equals ``model_draw`` on its pixels."""
    from meteor_demod_amd import map as M, overlay as O
    rows = 40
    keep = np.random.default_rng(12).random((rows, 3, 14)) >= 0.15
    place, info = MU.packets(rows, MU.mid_latitude_s0(40.0), keep=keep)
    images, filled = PU.pixels(rows, 9), MU.filled_of(place, rows)
    for select in ((2, 1, 0), (1,)):
        m = M.compose(MU.tle_text(), images, filled, place, info, select, device=gpu_device, px_per_deg=40)
        styles = O.default_styles(width=2.0)
        styles[1].inside_only = True
        layers = [(_coast(m, 4), 0), (O.graticule(m, "auto"), 1)]
        got, rep = O.draw_map(m, layers, styles, device=gpu_device)
        want = O.model_draw(m.pixels, m, layers, styles, m.valid)
        print(f"select {select}: {m.pixels.shape}, {rep}")
        assert got.shape == m.pixels.shape and np.array_equal(got, want) and (got != m.pixels).any() and rep.pixels[0] > 0


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_overlay(tmp_path, gpu_device):
    """The one-row recording under two names through --image --composite 321 --map --mosaic with --graticule 5 --overlay coast.txt:
    every _map_overlay.ppm and the _mosaic_overlay.ppm are the Python pipeline's bytes, with world files of the same six lines; the
    plain maps, the mosaic and their world files are those of a run without the two options, byte for byte."""
    import frames_util as U
    from conftest import GOLDEN, ROOT
    from meteor_demod_amd import image, map as M, mosaic as Z, overlay as O, rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    tle = GOLDEN / "map_tle.txt"
    st, iq = MU.recording()
    dirs = [tmp_path / "with", tmp_path / "plain"]
    for d in dirs:
        d.mkdir()
        for name in ("one.wav", "two.wav"):
            (d / name).write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    # strokes all over the globe, 2 degrees apart: whatever ground the pass saw, some cross it
    coast = tmp_path / "coast.txt"
    coast.write_text("# strokes\n" + "\n".join(f"{k} -80\n{k + 30 if k + 30 <= 180 else k + 30 - 360}, 80\n" for k in range(-180, 180, 2)))
    common = ("--cadu", "--image", "--composite", "321", "--map", str(tle), "--map-scale", "60", "--scan-angle", "108", "--mosaic", "both")

    def run(cwd, *flags):
        return subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), *common, *flags, "one.wav", "two.wav"], capture_output=True, text=True, cwd=cwd, timeout=300)
    p = run(dirs[0], "--graticule", "5", "--overlay", str(coast), "--overlay-colour", "ff8000", "--overlay-width", "1.5")
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    q = run(dirs[1])
    assert q.returncode == 0, q.stderr
    plain = ("one.wav_321_map", "two.wav_321_map", "both_321_mosaic")
    for stem in plain:
        for ext in (".ppm", ".wld"):
            assert (dirs[0] / (stem + ext)).read_bytes() == (dirs[1] / (stem + ext)).read_bytes(), stem + ext
        assert (dirs[0] / (stem + "_overlay.wld")).read_text() == (dirs[0] / (stem + ".wld")).read_text()
    assert not list(dirs[1].glob("*overlay*")) and [l for l in p.stdout.splitlines() if "_overlay: " not in l] == q.stdout.splitlines()
    cadu = np.frombuffer((dirs[0] / "one.wav.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    styles, vectors = O.default_styles(colour=(255, 128, 0), width=1.5), O.read_vectors(coast)
    one = M.image_to_map(res, tle.read_text(), composite="321", device=gpu_device, px_per_deg=60, scan_deg=108)
    both = Z.images_to_mosaic([res, res], tle.read_text(), composite="321", device=gpu_device, px_per_deg=60, scan_deg=108)
    lines = [l for l in p.stdout.splitlines() if "_overlay: " in l]
    assert len(lines) == 3
    for stem, m, line in zip(plain, (one, one, both), lines):
        want, rep = O.draw_map(m, [(vectors, 0), (O.graticule(m, 5), 1)], styles, device=gpu_device)
        got = _pnm(dirs[0] / (stem + "_overlay.ppm"), rb"P6", 3)
        assert np.array_equal(got, want) and (want != m.pixels).any(), stem
        f = re.fullmatch(r"(\S*)" + re.escape(stem) + r"_overlay: (\d+) pieces kept, (\d+) tiles touched; lines: (\d+) pieces, (\d+) pixels; graticule: (\d+) pieces, (\d+) pixels", line)
        assert f, line
        assert [int(f.group(k)) for k in range(2, 8)] == [sum(rep.pieces), rep.tiles, rep.pieces[0], rep.pixels[0], rep.pieces[1], rep.pixels[1]] and rep.pixels[0] > 0
    # a grey map per channel takes the first colour byte; --graticule auto alone
    g = subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), "--image", "--map", str(tle), "--map-scale", "40", "--graticule", "auto", "-o", "grey.s", "one.wav"],
                       capture_output=True, text=True, cwd=dirs[0], timeout=300)
    assert g.returncode == 0, g.stderr
    for k, a in enumerate((64, 65, 66)):
        m = M.image_to_map(res, tle.read_text(), composite=str(k + 1), device=gpu_device, px_per_deg=40)
        want, rep = O.draw_map(m, [(O.graticule(m, "auto"), 1)], O.default_styles(), device=gpu_device)
        assert np.array_equal(_pnm(dirs[0] / f"grey_{a}_map_overlay.pgm", rb"P5", 1), want) and np.array_equal(_pnm(dirs[0] / f"grey_{a}_map.pgm", rb"P5", 1), m.pixels)
    assert g.stdout.count("_map_overlay: ") == 3
