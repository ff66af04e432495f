"""GPU tests of the mosaic layer (include/meteor_demod_amd_mosaic.h): the blend kernel against the host model, byte for byte, pixels,
valid and cover, on the hand-made passes of mosaic_util.py (1, 2, 3 and 8 passes of 3 and 5 strip rows under masks with holes and an
empty slot, outputs from 4 x 1 to 200 x 150, grey and colour, every selection, both modes), one pass against the map layer's warp,
inside canaries and garbage; the device entry's argument checks; the whole-mosaic entry in bands against the model on the two-pass
scene of test_mosaic_host.py; the C host's --mosaic.  Every GPU step runs once; every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

import map_util as MU
import mosaic_util as Z
from test_gpu_map import SELECTS, _dev, _pnm, _stream_handle

pytestmark = pytest.mark.gpu

KINDS = ("mixed", "empty1")
MODES = (Z.FEATHER, Z.BEST)
COUNTS = (1, 2, 3, 8)


def _dev_sources(src, gpu_device):
    """The passes of mosaic_util.sources on the device (tables and nodes stay numpy: blend copies them)."""
    return [None if s is None else ([_dev(x, gpu_device) for x in s[0]], [_dev(x, gpu_device) for x in s[1]], s[2], s[3]) for s in src]


@functools.lru_cache(maxsize=None)
def _want(kind, w, h, n, select, mode):
    from meteor_demod_amd import mosaic as M
    return M.model_blend(Z.sources(kind, w, h, n, len(select)), select, w, h, mode, valid=True, cover=True)


# ------------------------------------------------------------------------------------------------------ kernel against model
@pytest.mark.parametrize("kind", KINDS)
def test_blend_equals_the_model(kind, gpu_device):
    """The whole hand-made matrix; with and without the optional outputs."""
    from meteor_demod_amd import mosaic as M
    for w, h in Z.SIZES:
        for n in COUNTS:
            bad = 0
            for select in SELECTS:
                src = _dev_sources(Z.sources(kind, w, h, n, len(select)), gpu_device)
                for mode in MODES:
                    want = _want(kind, w, h, n, select, mode)
                    got = M.blend(src, select, w, h, mode, valid=True, cover=True)
                    alone = M.blend(src, select, w, h, mode)                                        # valid = cover = NULL
                    only_cover = M.blend(src, select, w, h, mode, cover=True)
                    bad += sum(int((a.cpu().numpy() != b).sum()) for a, b in zip(got, want)) + int((alone.cpu().numpy() != want[0]).sum())
                    bad += int((only_cover[0].cpu().numpy() != want[0]).sum()) + int((only_cover[1].cpu().numpy() != want[2]).sum())
            print(f"{kind}, {w} x {h}, {n} passes: {bad} bytes differ")
            assert bad == 0


def test_sizes_that_are_no_multiple_of_the_tile(gpu_device):
    """The cases of map_util.warp_cases (widths and heights that are no multiples of 16 or 32), each with a shifted copy of itself
    as a second pass of 5 strip rows."""
    from meteor_demod_amd import mosaic as M
    for name, w, h, nodes in MU.warp_cases():
        second = nodes.astype(np.int64) + np.where(nodes == MU.NO_NODE, 0, 300)
        a, b = Z.pass_data("mixed", 3, 0), Z.pass_data("mixed", 5, 1)
        bad = 0
        for select in ((2, 1, 0), (1,)):
            src = [(a[0], a[1], a[2][: len(select)], nodes), (b[0], b[1], b[2][: len(select)], second.astype(np.int32))]
            for mode in MODES:
                want = M.model_blend(src, select, w, h, mode, valid=True, cover=True)
                got = M.blend(_dev_sources(src, gpu_device), select, w, h, mode, valid=True, cover=True)
                bad += sum(int((x.cpu().numpy() != y).sum()) for x, y in zip(got, want))
        print(f"{name}: {w} x {h}, {bad} bytes differ")
        assert bad == 0


def test_one_pass_is_the_map_layers_warp(gpu_device):
    from meteor_demod_amd import map as MP, mosaic as M
    images, filled, luts = Z.pass_data("mixed", 3, 0)
    d_images, d_filled = [_dev(x, gpu_device) for x in images], [_dev(x, gpu_device) for x in filled]
    for name, w, h, nodes in MU.warp_cases():
        for select in ((2, 1, 0), (1,)):
            want, want_val = MP.warp(d_images, d_filled, select, luts[: len(select)], nodes, w, h, valid=True)
            for mode in MODES:
                out, val, cov = M.blend([(d_images, d_filled, luts[: len(select)], nodes)], select, w, h, mode, valid=True, cover=True)
                assert bool((out == want).all()) and bool((val == want_val).all()) and bool((cov == (want_val != 0)).all()), (name, select, mode)


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """Every pass's inputs inside garbage on both sides: the results are those of the inputs alone.  The outputs between canaries:
    they survive.  The inputs are only read."""
    import torch
    from meteor_demod_amd import mosaic as M
    w, h, select, n = 200, 150, (2, 0, 1), 3
    src = Z.sources("mixed", w, h, 4, 3)
    src = [src[0], src[1], src[3]]                                                    # (without the pass that has no nodes)
    rng = np.random.default_rng(shift)
    gap, parts = 2048, []
    for images, filled, luts, nodes in src:
        parts += [x.reshape(-1) for x in images] + [x.reshape(-1) for x in filled] + [luts.reshape(-1), nodes.reshape(-1).view(np.uint8)]
    buf = rng.integers(0, 256, gap + sum(p.size + gap + 4 for p in parts) + shift + 64, dtype=np.uint8)
    at, offs = gap + shift, []
    for part in parts:
        buf[at: at + part.size] = part
        offs.append(at)
        at += (part.size + gap + 3) // 4 * 4
    d = _dev(buf, gpu_device)
    base = d.data_ptr()
    assert base % 4 == 0
    arr = (M.MdemodMosaicSource * n)()
    for k, (images, filled, luts, nodes) in enumerate(src):
        o = offs[8 * k: 8 * k + 8]
        for s in range(3):
            arr[k].image[s], arr[k].filled[s] = base + o[s], base + o[3 + s]
        arr[k].lut, arr[k].nodes, arr[k].rows = base + o[6], base + o[7], images[0].shape[0] // 8
    pad = 64 + shift
    out = torch.full((pad + h * w * 3 + 64,), 0x5A, dtype=torch.uint8, device=d.device)
    val = torch.full((pad + h * w + 64,), 0xC3, dtype=torch.uint8, device=d.device)
    cov = torch.full((pad + h * w + 64,), 0x3C, dtype=torch.uint8, device=d.device)
    sel = (C.c_uint32 * 3)(*select)
    for mode in MODES:
        want = M.model_blend(src, select, w, h, mode, valid=True, cover=True)
        assert M.lib().mdemod_mosaic_blend_device(arr, n, sel, 3, mode, w, h, C.c_void_p(out.data_ptr() + pad), C.c_void_p(val.data_ptr() + pad),
                                                  C.c_void_p(cov.data_ptr() + pad), gpu_device, _stream_handle(gpu_device)) == 0
        o, v, c = out.cpu().numpy(), val.cpu().numpy(), cov.cpu().numpy()
        print(f"shift {shift}, blend {mode}: canaries of {pad} and 64 bytes around {o.size - pad - 64}, {v.size - pad - 64} and {c.size - pad - 64} bytes")
        for x, canary in ((o, 0x5A), (v, 0xC3), (c, 0x3C)):
            assert (x[:pad] == canary).all() and (x[-64:] == canary).all()
        assert np.array_equal(o[pad:-64].reshape(h, w, 3), want[0]) and np.array_equal(v[pad:-64].reshape(h, w), want[1]) and np.array_equal(c[pad:-64].reshape(h, w), want[2])
        assert ((want[2] & (want[2] - 1)) != 0).sum() > 0.3 * w * h or mode == Z.BEST
    assert np.array_equal(d.cpu().numpy(), buf)


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    """Every refusal with its text, and nothing written; n = 0 and height = 0 are nothing to do; a pass of no rows is empty and none
    of its pointers is looked at; two runs give the same bytes."""
    import torch
    from meteor_demod_amd import _capi, mosaic as M
    lib, st = M.lib(), _stream_handle(gpu_device)
    w, h, n = 200, 150, 2
    src = Z.sources("mixed", w, h, n, 3)
    n_nodes = src[0][3].size * 4
    sizes = []
    for images, filled, luts, nodes in src:
        rows = images[0].shape[0] // 8
        sizes.append((8 * rows * 1568, (rows * 14 + 3) // 4 * 4, rows))
    size = sum(3 * a + 3 * b + 768 + n_nodes for a, b, _ in sizes) + h * w * 5
    buf = torch.zeros(size + 64, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    at, where = base, []
    for (n_img, n_fil, rows), (images, filled, luts, nodes) in zip(sizes, src):
        a_img = [at + k * n_img for k in range(3)]
        a_fil = [at + 3 * n_img + k * n_fil for k in range(3)]
        a_lut = a_fil[2] + n_fil
        a_nodes = a_lut + 768
        for k in range(3):
            buf[a_img[k] - base: a_img[k] - base + n_img] = _dev(images[k].reshape(-1), gpu_device)
            buf[a_fil[k] - base: a_fil[k] - base + rows * 14] = _dev(filled[k].reshape(-1), gpu_device)
        buf[a_lut - base: a_lut - base + 768] = _dev(luts.reshape(-1), gpu_device)
        buf[a_nodes - base: a_nodes - base + n_nodes] = _dev(nodes.reshape(-1).view(np.uint8), gpu_device)
        where.append(dict(img=a_img, fil=a_fil, lut=a_lut, nd=a_nodes, rows=rows, n_img=n_img))
        at = a_nodes + n_nodes
    a_out, a_val, a_cov = at, at + h * w * 3, at + h * w * 4
    sel3, sel1 = (C.c_uint32 * 3)(2, 1, 0), (C.c_uint32 * 1)(1)

    def blend(passes=None, count=None, sel=sel3, planes=3, mode=0, width=w, height=h, out=a_out, val=a_val, cov=a_cov, last=None):
        passes = [dict(p) for p in (where if passes is None else passes)]
        if last:
            passes[-1].update(last)
        arr = (M.MdemodMosaicSource * max(len(passes), 1))()
        for k, p in enumerate(passes):
            for s in range(3):
                arr[k].image[s], arr[k].filled[s] = p["img"][s] or None, p["fil"][s] or None
            arr[k].lut, arr[k].nodes, arr[k].rows = p["lut"] or None, p["nd"] or None, p["rows"]
        return lib.mdemod_mosaic_blend_device(arr if count != -1 else None, len(passes) if count in (None, -1) else count, sel, planes, mode, width, height,
                                              C.c_void_p(out), C.c_void_p(val), C.c_void_p(cov), gpu_device, st)

    assert blend() == 0
    first = buf.cpu().numpy()
    want = M.model_blend(src, (2, 1, 0), w, h, 0, valid=True, cover=True)
    o = a_out - base
    assert np.array_equal(first[o: o + h * w * 3].reshape(h, w, 3), want[0]) and np.array_equal(first[o + h * w * 3: o + h * w * 4].reshape(h, w), want[1])
    assert np.array_equal(first[o + h * w * 4: o + h * w * 5].reshape(h, w), want[2])
    assert blend() == 0
    assert np.array_equal(buf.cpu().numpy(), first)                                # two runs: the same bytes
    # nothing to do: no pointer is looked at
    assert blend(count=0, out=0, val=0, cov=0) == 0 and blend(height=0, out=0) == 0
    # an empty pass: none of its pointers is looked at, and the result is that of the other pass
    empty = dict(img=[0, 0, 0], fil=[0, 0, 0], lut=0, nd=0, rows=0)
    assert blend(passes=[where[0], empty]) == 0
    one = M.model_blend(src[:1], (2, 1, 0), w, h, 0)
    assert np.array_equal(buf.cpu().numpy()[o: o + h * w * 3].reshape(h, w, 3), one)
    # only the selected slots are looked at
    assert blend(passes=[dict(where[k], img=[0, where[k]["img"][1], 0], fil=[0, where[k]["fil"][1], 0]) for k in range(2)], sel=sel1, planes=1, val=0, cov=0) == 0
    buf[o: o + h * w * 5] = 0xEE
    before = buf.cpu().numpy()
    l = where[-1]
    for word, change in (("planes", dict(planes=2)), ("selection", dict(sel=None)), ("slot", dict(sel=(C.c_uint32 * 3)(0, 3, 1))), ("more than a mosaic takes", dict(passes=[where[0]] * 9)),
                         ("needed", dict(count=-1)), ("blend", dict(mode=2)), ("65536", dict(last=dict(rows=65537))),
                         ("width", dict(width=w - 2)), ("width", dict(width=0)), ("width", dict(width=8196)), ("height", dict(height=16385)),
                         ("slot 2 of pass 1", dict(last=dict(img=[l["img"][0], l["img"][1], 0]))), ("slot 1 of pass 1", dict(last=dict(fil=[l["fil"][0], 0, l["fil"][2]]))),
                         ("of pass 1 are needed", dict(last=dict(lut=0))), ("of pass 1 are needed", dict(last=dict(nd=0))), ("needed", dict(out=0)),
                         ("multiples of 4", dict(out=a_out + 2)), ("multiples of 4", dict(val=a_val + 1)), ("multiples of 4", dict(cov=a_cov + 3)),
                         ("multiples of 4", dict(last=dict(lut=l["lut"] + 1))), ("multiples of 4", dict(last=dict(nd=l["nd"] + 2))),
                         ("multiples of 4", dict(last=dict(img=[l["img"][0] + 2, l["img"][1], l["img"][2]]))),
                         ("intersect", dict(out=l["img"][0] + 4)), ("intersect", dict(out=l["nd"] - h * w * 3 + 4)), ("intersect", dict(val=l["lut"])),
                         ("intersect", dict(val=a_out + 4)), ("intersect", dict(cov=a_val + 4)), ("intersect", dict(cov=a_out)),
                         ("intersect", dict(out=l["fil"][1] - h * w * 3 + 4)), ("intersect", dict(cov=where[0]["img"][2] + where[0]["n_img"] - 4))):
        rc = blend(**change)
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(buf.cpu().numpy(), before)                               # nothing was written


# ---------------------------------------------------------------------------------------------------------------- bands
@pytest.mark.parametrize("mode", MODES)
def test_compose_host_in_bands_equals_the_model(mode, gpu_device):
    """mdemod_mosaic_compose_host on the two-pass scene of test_mosaic_host.py in bands of 16, 48 and 1024 lines: the bytes of the
    model's host entry, with grid, timing, limits and counts; and the scene's squares are where the ground is."""
    import test_map_host as H
    import test_mosaic_host as TH
    from meteor_demod_amd import mosaic as M
    passes, marked = TH.e2e_passes()
    model = TH.e2e_model(mode)
    for piece in (16, 48, 1024):
        g = M.compose(passes, (2, 1, 0), device=gpu_device, stretch=0, px_per_deg=50, blend=mode, piece_lines=piece)
        assert np.array_equal(g.pixels, model.pixels) and np.array_equal(g.valid, model.valid) and np.array_equal(g.cover, model.cover), piece
        assert (g.sx, g.sy, g.lat_top, g.lon_left, g.blend, g.valid_pixels, g.overlap_pixels) == \
               (model.sx, model.sy, model.lat_top, model.lon_left, model.blend, model.valid_pixels, model.overlap_pixels)
        assert g.passes == model.passes
    print(f"{g.width} x {g.height}, {100 * g.valid_share:.1f} % valid, {100 * g.overlap_share:.1f} % in two bits of cover")
    H.check_scene(g, marked, f"GPU, blend {mode}")


def test_compose_host_stretches(gpu_device):
    """The three stretch settings, grey and colour, against the model's host entry (the histograms come from the device here)."""
    import test_mosaic_host as TH
    from meteor_demod_amd import _capi, mosaic as M
    passes = TH.stretch_passes()
    for select, opts in (((2, 1, 0), dict(px_per_deg=30, stretch=1)), ((1,), dict(px_per_deg=30, stretch=2, clip_low=100, clip_high=20, blend="best")),
                         ((0, 0, 2), dict(px_per_deg=30, stretch=1, side=-1))):
        model = M.model_host(passes, select, **opts)
        g = M.compose(passes, select, device=gpu_device, piece_lines=64, **opts)
        print(f"select {select}, {opts}: {g.pixels.shape}, limits {[r.limits for r in g.passes]}")
        assert np.array_equal(g.pixels, model.pixels) and np.array_equal(g.valid, model.valid) and np.array_equal(g.cover, model.cover) and g.passes == model.passes
    for word, opts in (("piece_lines", dict(piece_lines=24)), ("scale", dict(px_per_deg=0.5)), ("stretch", dict(stretch=3)), ("blend", dict(blend=2))):
        with pytest.raises(_capi.MdemodError) as e:
            M.compose(passes, (2, 1, 0), device=gpu_device, **opts)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_mosaic(tmp_path, gpu_device):
    """The one-row recording with real stamps under two names through --image --composite 321 --map --mosaic: the per-file maps are
    those of a run without --mosaic; the mosaic's .ppm, .wld and line are those of mosaic.images_to_mosaic on the same data, and the
    bytes are the single pass's map (two identical passes feather to themselves); without --composite one grey mosaic per channel."""
    import frames_util as U
    from conftest import GOLDEN, ROOT
    from meteor_demod_amd import image, mosaic as M, rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    tle = GOLDEN / "map_tle.txt"
    st, iq = MU.recording()
    for name in ("one.wav", "two.wav"):
        (tmp_path / name).write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    alone = tmp_path / "alone"
    alone.mkdir()
    (alone / "one.wav").write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))

    def run(cwd, files, *flags):
        return subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), *flags, *files], capture_output=True, text=True, cwd=cwd, timeout=300)

    common = ("--cadu", "--image", "--composite", "321", "--map", str(tle), "--map-scale", "60", "--scan-angle", "108")
    p = run(tmp_path, ["one.wav", "two.wav"], *common, "--mosaic", "both")
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    q = run(alone, ["one.wav"], *common, "-o", "one.wav.s")                            # (the name a run of several files gives it)
    assert q.returncode == 0, q.stderr
    single = (alone / "one.wav_321_map.ppm").read_bytes()
    for name in ("one", "two"):
        assert (tmp_path / f"{name}.wav_321_map.ppm").read_bytes() == single
        assert (tmp_path / f"{name}.wav_321_map.wld").read_text() == (alone / "one.wav_321_map.wld").read_text()
    assert [l for l in p.stdout.splitlines() if l.startswith("one.wav")] == [l for l in q.stdout.splitlines() if l.startswith("one.wav")]
    cadu = np.frombuffer((tmp_path / "one.wav.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    want = M.images_to_mosaic([res, res], tle.read_text(), composite="321", device=gpu_device, px_per_deg=60, scan_deg=108)
    got = _pnm(tmp_path / "both_321_mosaic.ppm", rb"P6", 3)
    assert np.array_equal(got, want.pixels) and want.valid.any() and np.array_equal(got, _pnm(alone / "one.wav_321_map.ppm", rb"P6", 3))
    assert np.array_equal(want.cover, 3 * (want.valid != 0))
    wld = (tmp_path / "both_321_mosaic.wld").read_text()
    assert [float(v) for v in wld.split()] == [float(v) for v in want.world_file().split()] and len(wld.split()) == 6
    m = re.fullmatch(r"both: mosaic 321 \(feather\): (\d+) x (\d+) at (\d+) x ([\d.]+) px/deg; lat ([-\d.]+) \.\. ([-\d.]+), lon ([-\d.]+) \.\. ([-\d.]+); "
                     r"(\d+) passes; first lines (\S+)Z, (\S+)Z; ([\d.]+) % of pixels valid; ([\d.]+) % seen by two or more passes", p.stdout.strip().splitlines()[-1])
    assert m, p.stdout
    assert [int(m.group(k)) for k in (1, 2, 3, 9)] == [want.width, want.height, want.sx, 2] and float(m.group(4)) == 60.0
    assert abs(float(m.group(6)) - want.lat_top) < 1e-4 and abs(float(m.group(7)) - want.lon_left) < 1e-4
    assert [m.group(10), m.group(11)] == [r.first_line_utc().isoformat(timespec="milliseconds") for r in want.passes]
    assert abs(float(m.group(12)) - 100 * want.valid_share) < 0.051 and abs(float(m.group(13)) - 100 * want.overlap_share) < 0.051 and want.overlap_share == want.valid_share
    # without --composite: one grey mosaic per channel; --mosaic-blend best
    g = run(tmp_path, ["one.wav", "two.wav"], "--image", "--map", str(tle), "--map-scale", "40", "--mosaic", "grey", "--mosaic-blend", "best")
    assert g.returncode == 0, g.stderr
    for k, a in enumerate((64, 65, 66)):
        one = M.images_to_mosaic([res, res], tle.read_text(), composite=str(k + 1), device=gpu_device, px_per_deg=40, blend="best")
        assert np.array_equal(_pnm(tmp_path / f"grey_{a}_mosaic.pgm", rb"P5", 1), one.pixels) and (tmp_path / f"grey_{a}_mosaic.wld").exists()
        assert set(np.unique(one.cover)) == {0, 1}
    assert g.stdout.count("grey: mosaic 6") == 3 and g.stdout.count("(best)") == 3 and not list(tmp_path.glob("grey*.ppm"))
