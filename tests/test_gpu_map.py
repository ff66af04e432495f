"""GPU tests of the map layer (include/meteor_demod_amd_map.h): the warp kernel against the host model, byte for byte, pixels and
valid, on the hand-made node grids of map_util.warp_cases (3 strip rows of random bytes under masks with holes and an empty slot,
outputs from 4 x 1 to 200 x 150, grey and colour, every selection), inside canaries and garbage; the device entry's argument
checks; the whole-map entry in bands against one batch and the model; the scene of test_map_host.py through the GPU path; the C host's
--map.  Every GPU step runs once; every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

import map_util as MU
import picture_util as PU

pytestmark = pytest.mark.gpu

SELECTS = ((2, 1, 0), (1,), (0, 0, 2), (0,), (2,), (1, 1, 1))
KINDS = ("mixed", "empty1")


def _dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{gpu_device}")


def _stream_handle(gpu_device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)


@functools.lru_cache(maxsize=None)
def _source(kind):
    return PU.pixels(MU.SRC_ROWS, 31), PU.masks(kind, MU.SRC_ROWS, 4), PU.random_luts(2)


@functools.lru_cache(maxsize=None)
def _want(kind):
    """The model's results of every case and selection, computed once."""
    from meteor_demod_amd import map as M
    images, filled, luts = _source(kind)
    return {(name, s): M.model_warp(images, filled, s, luts[: len(s)], nodes, w, h, valid=True) for name, w, h, nodes in MU.warp_cases() for s in SELECTS}


# ------------------------------------------------------------------------------------------------------ kernel against model
@pytest.mark.parametrize("kind", KINDS)
def test_warp_equals_the_model(kind, gpu_device):
    """Every case of map_util.warp_cases under masks with holes ('mixed') and with slot 1 empty ('empty1'), planes 3 and 1, every
    slot and a repeated one; with and without the valid output."""
    from meteor_demod_amd import map as M
    images, filled, luts = _source(kind)
    d_images, d_filled = [_dev(x, gpu_device) for x in images], [_dev(x, gpu_device) for x in filled]
    for name, w, h, nodes in MU.warp_cases():
        bad = 0
        for s in SELECTS:
            want, want_val = _want(kind)[(name, s)]
            out, val = M.warp(d_images, d_filled, s, luts[: len(s)], nodes, w, h, valid=True)
            alone = M.warp(d_images, d_filled, s, luts[: len(s)], nodes, w, h)                                # valid = NULL
            bad += int((out.cpu().numpy() != want).sum()) + int((val.cpu().numpy() != want_val).sum()) + int((alone.cpu().numpy() != want).sum())
        print(f"{kind}, {name}: {w} x {h}, {np.count_nonzero(want_val)} of {want_val.size} valid, {bad} bytes differ")
        assert bad == 0


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """The inputs inside garbage on both sides: the results are those of the inputs alone.  The outputs between canaries: they
    survive.  The inputs are only read."""
    import torch
    from meteor_demod_amd import map as M
    images, filled, luts = _source("mixed")
    select = (2, 0, 1)
    for name in ("magnified 8 times", "any int32 in the nodes", "rotated 90 degrees"):
        _, w, h, nodes = next(c for c in MU.warp_cases() if c[0] == name)
        want, want_val = M.model_warp(images, filled, select, luts, nodes, w, h, valid=True)
        rng = np.random.default_rng(shift)
        rows = MU.SRC_ROWS
        sizes = [8 * rows * 1568] * 3 + [rows * 14] * 3 + [768, nodes.size * 4]
        parts = [x.reshape(-1) for x in images] + [x.reshape(-1) for x in filled] + [luts.reshape(-1), nodes.reshape(-1).view(np.uint8)]
        gap = 2048
        buf = rng.integers(0, 256, gap + sum(s + gap + 4 for s in sizes) + shift + 64, dtype=np.uint8)
        at, offs = gap + shift, []
        for s, part in zip(sizes, parts):
            buf[at: at + s] = part
            offs.append(at)
            at += (s + gap + 3) // 4 * 4
        d = _dev(buf, gpu_device)
        base = d.data_ptr()
        assert base % 4 == 0
        slots, cells = M._SLOTS(*[base + o for o in offs[:3]]), M._SLOTS(*[base + o for o in offs[3:6]])
        pad = 64 + shift
        out = torch.full((pad + h * w * 3 + 64,), 0x5A, dtype=torch.uint8, device=d.device)
        val = torch.full((pad + h * w + 64,), 0xC3, dtype=torch.uint8, device=d.device)
        sel = (C.c_uint32 * 3)(*select)
        assert M.lib().mdemod_map_warp_device(C.byref(slots), C.byref(cells), rows, sel, 3, C.c_void_p(base + offs[6]), C.c_void_p(base + offs[7]), w, h,
                                              C.c_void_p(out.data_ptr() + pad), C.c_void_p(val.data_ptr() + pad), gpu_device, _stream_handle(gpu_device)) == 0
        o, v = out.cpu().numpy(), val.cpu().numpy()
        print(f"shift {shift}, {name}: canaries of {pad} and 64 bytes around {o.size - pad - 64} and {v.size - pad - 64} bytes")
        assert (o[:pad] == 0x5A).all() and (o[-64:] == 0x5A).all() and (v[:pad] == 0xC3).all() and (v[-64:] == 0xC3).all()
        assert np.array_equal(o[pad:-64].reshape(h, w, 3), want) and np.array_equal(v[pad:-64].reshape(h, w), want_val)
        assert np.array_equal(d.cpu().numpy(), buf)


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    """Every refusal with its text, and nothing written; rows = 0 and height = 0 are nothing to do; two runs give the same bytes."""
    import torch
    from meteor_demod_amd import _capi, map as M
    lib, st = M.lib(), _stream_handle(gpu_device)
    images, filled, luts = _source("mixed")
    rows = MU.SRC_ROWS
    _, w, h, nodes = next(c for c in MU.warp_cases() if c[0] == "magnified 8 times")
    n_img, n_fil, n_nodes = 8 * rows * 1568, 44, nodes.size * 4                     # (42 bytes of masks in 44)
    size = 3 * n_img + 3 * n_fil + 768 + n_nodes + h * w * 3 + h * w
    buf = torch.zeros(size + 64, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    a_img = [base + k * n_img for k in range(3)]
    a_fil = [base + 3 * n_img + k * n_fil for k in range(3)]
    a_lut = a_fil[2] + n_fil
    a_nodes = a_lut + 768
    a_out = a_nodes + n_nodes
    a_val = a_out + h * w * 3
    for k in range(3):
        buf[a_img[k] - base: a_img[k] - base + n_img] = _dev(images[k].reshape(-1), gpu_device)
        buf[a_fil[k] - base: a_fil[k] - base + 42] = _dev(filled[k].reshape(-1), gpu_device)
    buf[a_lut - base: a_lut - base + 768] = _dev(luts.reshape(-1), gpu_device)
    buf[a_nodes - base: a_nodes - base + n_nodes] = _dev(nodes.reshape(-1).view(np.uint8), gpu_device)
    sel3, sel1 = (C.c_uint32 * 3)(2, 1, 0), (C.c_uint32 * 1)(1)

    def warp(img, fil, r, sel, planes, lut, nd, width, height, out, val):
        return lib.mdemod_map_warp_device(C.byref(M._SLOTS(*img)) if img else None, C.byref(M._SLOTS(*fil)) if fil else None, r, sel, planes, C.c_void_p(lut),
                                          C.c_void_p(nd), width, height, C.c_void_p(out), C.c_void_p(val), gpu_device, st)

    good = dict(img=a_img, fil=a_fil, r=rows, sel=sel3, planes=3, lut=a_lut, nd=a_nodes, width=w, height=h, out=a_out, val=a_val)
    assert warp(**good) == 0
    first = buf.cpu().numpy()
    want, want_val = M.model_warp(images, filled, (2, 1, 0), luts, nodes, w, h, valid=True)
    assert np.array_equal(first[a_out - base: a_val - base].reshape(h, w, 3), want) and np.array_equal(first[a_val - base: a_val - base + h * w].reshape(h, w), want_val)
    assert warp(**good) == 0
    assert np.array_equal(buf.cpu().numpy(), first)                                # two runs: the same bytes
    # nothing to do: no pointer is looked at
    assert warp(None, None, 0, sel3, 3, 0, 0, w, h, 0, 0) == 0 and warp(**{**good, "height": 0, "out": 0, "nd": 0}) == 0
    # only the selected slots are looked at
    assert warp([0, a_img[1], 0], [0, a_fil[1], 0], rows, sel1, 1, a_lut, a_nodes, w, h, a_out, 0) == 0
    buf[a_out - base: a_out - base + h * w * 3 + h * w] = 0xEE
    before = buf.cpu().numpy()
    for word, change in (("planes", dict(planes=2)), ("selection", dict(sel=None)), ("slot", dict(sel=(C.c_uint32 * 3)(0, 3, 1))), ("65536", dict(r=65537)),
                         ("width", dict(width=w - 2)), ("width", dict(width=0)), ("width", dict(width=8196)), ("height", dict(height=16385)),
                         ("slot 2", dict(img=[a_img[0], a_img[1], 0])), ("slot 1", dict(fil=[a_fil[0], 0, a_fil[2]])), ("needed", dict(img=None)),
                         ("needed", dict(lut=0)), ("needed", dict(nd=0)), ("needed", dict(out=0)),
                         ("multiples of 4", dict(out=a_out + 2)), ("multiples of 4", dict(val=a_val + 1)), ("multiples of 4", dict(lut=a_lut + 1)),
                         ("multiples of 4", dict(nd=a_nodes + 2)), ("multiples of 4", dict(img=[a_img[0] + 2, a_img[1], a_img[2]])),
                         ("intersect", dict(out=a_img[0] + 4)), ("intersect", dict(out=a_nodes - h * w * 3 + 4)), ("intersect", dict(val=a_lut)),
                         ("intersect", dict(val=a_out + 4)), ("intersect", dict(out=a_fil[1] - h * w * 3 + 4)), ("intersect", dict(val=a_nodes + n_nodes - 4))):
        rc = warp(**{**good, **change})
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(buf.cpu().numpy(), before)                               # nothing was written


# ---------------------------------------------------------------------------------------------------------------- bands
def test_compose_host_in_bands_equals_one_batch(gpu_device):
    """mdemod_map_compose_host on a synthetic pass of 40 strip rows in bands of 16, 48 and 1024 lines: the same bytes, and the
    bytes of the model fed the same tables and nodes (the model's host entry: the same time fit, grid and tables)."""
    from meteor_demod_amd import _capi, map as M
    rows = 40
    rng = np.random.default_rng(12)
    keep = rng.random((rows, 3, 14)) >= 0.15
    place, info = MU.packets(rows, MU.mid_latitude_s0(40.0), keep=keep)
    images, filled = PU.pixels(rows, 9), MU.filled_of(place, rows)
    for select, opts in (((2, 1, 0), dict(px_per_deg=40)), ((1,), dict(px_per_deg=25, clip_low=100, clip_high=0)), ((0, 0, 2), dict(px_per_deg=40, stretch=0, side=-1))):
        model = M.model_host(MU.tle_text(), images, filled, place, info, select, **opts)
        got = [M.compose(MU.tle_text(), images, filled, place, info, select, device=gpu_device, piece_lines=p, **opts) for p in (16, 48, 1024)]
        print(f"select {select}, {opts}: {model.pixels.shape}, limits {model.limits}, {100 * model.valid_share:.1f} % valid")
        assert model.height > 48 and 0.2 < model.valid_share < 1.0
        for g in got:
            assert np.array_equal(g.pixels, model.pixels) and np.array_equal(g.valid, model.valid) and g.limits == model.limits
            assert (g.sx, g.sy, g.lat_top, g.lon_left, g.row_period, g.rows_fit, g.date, g.utc0) == \
                   (model.sx, model.sy, model.lat_top, model.lon_left, model.row_period, model.rows_fit, model.date, model.utc0)
    for word, opts in (("piece_lines", dict(piece_lines=24)), ("scale", dict(px_per_deg=0.5)), ("clips", dict(clip_low=500)), ("time offset", dict(time_offset=1e6))):
        with pytest.raises(_capi.MdemodError) as e:
            M.compose(MU.tle_text(), images, filled, place, info, (2, 1, 0), device=gpu_device, **opts)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail


def test_scene_through_the_gpu_path(gpu_device):
    """The scene of test_map_host.py: every valid pixel at least 3 output pixels from a square's edge has exactly its square's level."""
    import test_map_host as H
    from meteor_demod_amd import map as M
    images, filled, place, info, ref, marked = H.e2e_case()
    m = M.compose(MU.tle_text(), images, filled, place, info, (2, 1, 0), device=gpu_device, stretch=0, px_per_deg=50)
    print(f"{m.width} x {m.height}, {100 * m.valid_share:.1f} % valid, marked square at {marked}")
    H.check_scene(m, marked, "GPU")


# ------------------------------------------------------------------------------------------------------------------- CLI
def _pnm(path, magic, planes):
    raw = path.read_bytes()
    m = re.match(magic + rb"\n(\d+) (\d+)\n255\n", raw)
    assert m, raw[:20]
    w, h = int(m.group(1)), int(m.group(2))
    assert len(raw) == m.end() + w * h * planes
    a = np.frombuffer(raw[m.end():], dtype=np.uint8)
    return a.reshape(h, w, 3) if planes == 3 else a.reshape(h, w)


def test_cli_map(tmp_path, gpu_device):
    """--image --composite 321 --map on the one-row recording with real stamps: the .ppm, the .wld and the line are those of
    map.image_to_map on the same data; without --composite one .pgm and .wld per channel; the refusals."""
    import frames_util as U
    from conftest import GOLDEN, ROOT
    from meteor_demod_amd import image, map as M, rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    tle = GOLDEN / "map_tle.txt"
    st, iq = MU.recording()
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))

    def run(name, *flags):
        return subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), *flags, "-o", str(tmp_path / name), str(wav)], capture_output=True,
                              text=True, cwd=tmp_path, timeout=300)

    p = run("pass.s", "--cadu", "--image", "--composite", "321", "--map", str(tle), "--map-scale", "60", "--scan-angle", "108")
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    cadu = np.frombuffer((tmp_path / "pass.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    want = M.image_to_map(res, tle.read_text(), composite="321", device=gpu_device, px_per_deg=60, scan_deg=108)
    got = _pnm(tmp_path / "pass_321_map.ppm", rb"P6", 3)
    assert np.array_equal(got, want.pixels) and want.valid.any()                   # (8 lines in a box of some 230: a few per cent)
    wld = (tmp_path / "pass_321_map.wld").read_text()
    assert [float(v) for v in wld.split()] == [float(v) for v in want.world_file().split()] and len(wld.split()) == 6
    m = re.fullmatch(r"(\S+)pass: map 321: (\d+) x (\d+) at (\d+) x ([\d.]+) px/deg; lat ([-\d.]+) \.\. ([-\d.]+), lon ([-\d.]+) \.\. ([-\d.]+); "
                     r"row period ([\d.]+) s over (\d+) rows; first line (\S+)Z; ([\d.]+) % of pixels valid", p.stdout.strip().splitlines()[-1])
    assert m, p.stdout
    assert [int(m.group(k)) for k in (2, 3, 4, 11)] == [want.width, want.height, want.sx, want.rows_fit] and float(m.group(5)) == 60.0
    assert abs(float(m.group(7)) - want.lat_top) < 1e-4 and abs(float(m.group(8)) - want.lon_left) < 1e-4 and abs(float(m.group(10)) - want.row_period) < 1e-6
    assert m.group(12) == want.first_line_utc().isoformat(timespec="milliseconds") and abs(float(m.group(13)) - 100 * want.valid_share) < 0.051
    assert want.rows_fit == 1 and want.row_period == 8 / 6.5 and want.date == 19822
    # without --composite: one grey map per channel
    q = run("grey.s", "--image", "--map", str(tle), "--map-scale", "40", "--scan-side", "-1", "--date", "2024-04-09", "--time-offset", "10800")
    assert q.returncode == 0, q.stderr
    for k, a in enumerate((64, 65, 66)):
        one = M.image_to_map(res, tle.read_text(), composite=str(k + 1), device=gpu_device, px_per_deg=40, side=-1, date="2024-04-09")
        assert np.array_equal(_pnm(tmp_path / f"grey_{a}_map.pgm", rb"P5", 1), one.pixels) and (tmp_path / f"grey_{a}_map.wld").exists()
    assert q.stdout.count(": map 6") == 3 and not list(tmp_path.glob("grey*.ppm"))
    junk = tmp_path / "junk.txt"
    junk.write_text("no element set here\n")
    for flags, word in ((("--map", str(tle)), "only with --image"), (("--image", "--map-scale", "50"), "only with --map"),
                        (("--image", "--map", str(tmp_path / "none.txt")), "could not read"), (("--image", "--map", str(junk)), "no element set"),
                        (("--image", "--map", str(tle), "--norad", "12345"), "catalogue number 12345"),
                        (("--image", "--map", str(tle), "--map-scale", "1001"), "1 .. 1000"), (("--image", "--map", str(tle), "--map-scale", "0"), "1 .. 1000"),
                        (("--image", "--map", str(tle), "--scan-side", "2"), "1 or -1"), (("--image", "--map", str(tle), "--date", "yesterday"), "yyyy-mm-dd"),
                        (("--image", "--map", str(tle), "--altitude", "800"), "only with --rectify"), (("--image", "--map", str(tle), "--scan-angle", "131"), "scan angle")):
        r = run("no.s", *flags)
        assert r.returncode == 1 and word in r.stderr and not (tmp_path / "no.s").exists(), (flags, r.stderr)
