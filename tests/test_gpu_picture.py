"""GPU tests of the picture layer (include/meteor_demod_amd_picture.h): both kernels against the host model, byte for byte, at the
smallest shapes that reach every path (1, 2 and 9 strip rows; every kind of mask; grey and colour; the default, the narrow and the
identity map) and at one output of more than 2^31 bytes; the histogram against numpy.bincount; guard regions; the entries' argument
checks; the whole-picture entry in pieces; the sender's picture through the image layer into a composite; and the C host's
--rectify / --composite.  Every GPU step runs once; every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

import frames_util as U
import image_util as I
import picture_util as PU

pytestmark = pytest.mark.gpu

KINDS = ("all", "none", "checker", "empty1", "mixed")
MAPS = (dict(), dict(rectify=0), dict(altitude_km=820, scan_deg=20))
SELECTS = ((2, 1, 0), (1,), (0, 0, 2))


def _dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{gpu_device}")


def _stream_handle(gpu_device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)


@functools.lru_cache(maxsize=None)
def _maps(k):
    from meteor_demod_amd import picture
    return picture.column_map(**MAPS[k])


@functools.lru_cache(maxsize=None)
def _case(rows, kind):
    """(pictures, masks, tables) and the model's results, computed once per case."""
    from meteor_demod_amd import picture
    images, filled, luts = PU.pixels(rows, 100 + rows), PU.masks(kind, rows, rows), PU.random_luts(rows)
    want = {(k, s): picture.model_render(images, filled, s, luts[: len(s)], _maps(k), valid=True) for k in range(len(MAPS)) for s in SELECTS}
    return images, filled, luts, want, picture.model_histogram(images, filled)


# ----------------------------------------------------------------------------------------------------- kernels against model
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", [1, 2, 9])
def test_render_equals_the_model(rows, kind, gpu_device):
    """Random pixels (garbage in the unfilled cells too) under every kind of mask; planes 3 and 1 and a repeated slot; the default
    map (W 2784: 696 quads, the third step of a block is partial), the identity (392 quads) and altitude 820 / scan 20 (W 1584,
    neighbouring outputs share taps); tables that are permutations, so 0 and 255 are reached; the valid output as well."""
    from meteor_demod_amd import picture
    images, filled, luts, want, _ = _case(rows, kind)
    d_images, d_filled = [_dev(x, gpu_device) for x in images], [_dev(x, gpu_device) for x in filled]
    for k in range(len(MAPS)):
        for s in SELECTS:
            out, val = picture.render(d_images, d_filled, s, luts[: len(s)], _maps(k), valid=True)
            out, val = out.cpu().numpy(), val.cpu().numpy()
            w_out, w_val = want[(k, s)]
            print(f"rows {rows}, {kind}, {MAPS[k] or 'default'}, select {s}: W {_maps(k).size}, {np.count_nonzero(val)} of {val.size} valid, "
                  f"bytes {out.min()} .. {out.max()}, {int((out != w_out).sum())} bytes differ")
            assert np.array_equal(out, w_out) and np.array_equal(val, w_val)
            alone = picture.render(d_images, d_filled, s, luts[: len(s)], _maps(k)).cpu().numpy()     # valid = NULL
            assert np.array_equal(alone, w_out)
    if kind == "all":
        assert out.min() == 0 and out.max() == 255


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", [1, 2, 9])
def test_histogram_equals_bincount(rows, kind, gpu_device):
    from meteor_demod_amd import picture
    images, filled, _, _, model = _case(rows, kind)
    want = PU.histogram(images, filled)
    got = picture.histogram([_dev(x, gpu_device) for x in images], [_dev(x, gpu_device) for x in filled]).cpu().numpy().view(np.uint32)
    print(f"rows {rows}, {kind}: {got.sum(axis=1).tolist()} pixels counted per slot, of {8 * rows * 1568}")
    assert np.array_equal(got, want) and np.array_equal(model, want)
    if rows == 2:                                                                   # a slot that is not given is not counted
        part = picture.histogram([_dev(images[0], gpu_device), None, _dev(images[2], gpu_device)], [_dev(filled[0], gpu_device), None, _dev(filled[2], gpu_device)])
        part = part.cpu().numpy().view(np.uint32)
        assert np.array_equal(part[[0, 2]], want[[0, 2]]) and not part[1].any()


def test_histogram_of_many_rows_crosses_the_grid(gpu_device):
    """1030 strip rows: more than the 1024 blocks of the grid, so some blocks walk two rows."""
    import torch
    from meteor_demod_amd import picture
    rows = 1030
    rng = np.random.default_rng(9)
    im = rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8)
    fl = (rng.random((rows, 14)) < 0.7).astype(np.uint8)
    got = picture.histogram([None, _dev(im, gpu_device), None], [None, _dev(fl, gpu_device), None]).cpu().numpy().view(np.uint32)
    want = PU.histogram([None, im, None], [None, fl, None])
    print(f"{rows} rows: {int(got[1].sum())} pixels counted, {int(fl.sum()) * 896} filled")
    assert np.array_equal(got, want)
    torch.cuda.synchronize(gpu_device)


def test_render_beyond_two_to_the_31_bytes(gpu_device):
    """33 000 strip rows of colour at the default width are 2.2 GB of output: a byte offset kept in 32 bits would wrap.  One slot
    made on the device shows in all three planes; the first and the last two strip rows come back and equal the model."""
    import torch
    from meteor_demod_amd import picture
    rows, select, cmap, luts = 33000, (0, 0, 0), _maps(0), PU.random_luts(4)
    gen = torch.Generator(device=f"cuda:{gpu_device}").manual_seed(3)
    im = torch.randint(0, 256, (8 * rows, 1568), dtype=torch.uint8, device=f"cuda:{gpu_device}", generator=gen)
    fl = (torch.rand((rows, 14), device=f"cuda:{gpu_device}", generator=gen) < 0.8).to(torch.uint8)
    out, val = picture.render([im, None, None], [fl, None, None], select, luts, cmap, valid=True)
    assert out.numel() > 1 << 31
    for at in (0, rows - 2):
        h_im, h_fl = im[8 * at: 8 * at + 16].cpu().numpy(), fl[at: at + 2].cpu().numpy()
        want, want_val = picture.model_render([h_im, None, None], [h_fl, None, None], select, luts, cmap, valid=True)
        got, got_val = out[8 * at: 8 * at + 16].cpu().numpy(), val[at: at + 2].cpu().numpy()
        print(f"strip rows {at}, {at + 1} of {rows}: output from byte {8 * at * cmap.size * 3}, {int((got != want).sum())} bytes differ")
        assert np.array_equal(got, want) and np.array_equal(got_val, want_val)


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """The inputs inside garbage on both sides: the results are those of the inputs alone.  The outputs between canaries: they
    survive.  The inputs are only read."""
    import torch
    from meteor_demod_amd import picture
    rows, select = 2, (2, 0, 1)
    images, filled, luts, _, model_hist = _case(rows, "mixed")
    cmap = _maps(0)
    w = cmap.size
    want, want_val = picture.model_render(images, filled, select, luts, cmap, valid=True)
    rng = np.random.default_rng(shift)
    sizes = [8 * rows * 1568] * 3 + [rows * 14] * 3 + [768, 4 * w]
    parts = [x.reshape(-1) for x in images] + [x.reshape(-1) for x in filled] + [luts.reshape(-1), cmap.view(np.uint8)]
    gap = 2048
    buf = rng.integers(0, 256, gap + sum(s + gap for s in sizes) + shift + 64, dtype=np.uint8)
    at, offs = gap + shift, []
    for s, part in zip(sizes, parts):
        buf[at: at + s] = part
        offs.append(at)
        at += (s + gap + 3) // 4 * 4
    d = _dev(buf, gpu_device)
    base = d.data_ptr()
    assert base % 4 == 0
    slots = picture._SLOTS(*[base + o for o in offs[:3]])
    cells = picture._SLOTS(*[base + o for o in offs[3:6]])
    pad = 64 + shift
    hist = torch.full((pad + 3072 + 64,), 0xA5, dtype=torch.uint8, device=d.device)
    out = torch.full((pad + 8 * rows * w * 3 + 64,), 0x5A, dtype=torch.uint8, device=d.device)
    val = torch.full((pad + rows * w + 64,), 0xC3, dtype=torch.uint8, device=d.device)
    st, lib = _stream_handle(gpu_device), picture.lib()
    assert lib.mdemod_picture_histogram_device(C.byref(slots), C.byref(cells), rows, C.c_void_p(hist.data_ptr() + pad), gpu_device, st) == 0
    sel = (C.c_uint32 * 3)(*select)
    assert lib.mdemod_picture_render_device(C.byref(slots), C.byref(cells), rows, sel, 3, C.c_void_p(base + offs[6]), C.c_void_p(base + offs[7]), w,
                                            C.c_void_p(out.data_ptr() + pad), C.c_void_p(val.data_ptr() + pad), gpu_device, st) == 0
    h, o, v = hist.cpu().numpy(), out.cpu().numpy(), val.cpu().numpy()
    print(f"shift {shift}: canaries of {pad} and 64 bytes around 3072, {o.size - pad - 64} and {v.size - pad - 64} bytes")
    assert (h[:pad] == 0xA5).all() and (h[-64:] == 0xA5).all() and (o[:pad] == 0x5A).all() and (o[-64:] == 0x5A).all()
    assert (v[:pad] == 0xC3).all() and (v[-64:] == 0xC3).all()
    assert np.array_equal(h[pad:-64].view(np.uint32).reshape(3, 256), model_hist)
    assert np.array_equal(o[pad:-64].reshape(8 * rows, w, 3), want) and np.array_equal(v[pad:-64].reshape(rows, w), want_val)
    assert np.array_equal(d.cpu().numpy(), buf)


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    import torch
    from meteor_demod_amd import _capi, picture
    lib, st = picture.lib(), _stream_handle(gpu_device)
    rows, w = 2, 1568
    images, filled, luts, want, _ = _case(rows, "mixed")
    cmap = _maps(1)
    n_img, n_fil = 8 * rows * 1568, 32                                             # (28 bytes of masks in 32)
    size = 3 * n_img + 3 * n_fil + 768 + 4 * w + 3072 + 8 * rows * w * 3 + rows * w
    buf = torch.zeros(size + 64, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    a_img = [base + k * n_img for k in range(3)]
    a_fil = [base + 3 * n_img + k * n_fil for k in range(3)]
    a_lut = a_fil[2] + n_fil
    a_map, a_hist = a_lut + 768, a_lut + 768 + 4 * w
    a_out = a_hist + 3072
    a_val = a_out + 8 * rows * w * 3
    for k in range(3):
        buf[a_img[k] - base: a_img[k] - base + n_img] = _dev(images[k].reshape(-1), gpu_device)
        buf[a_fil[k] - base: a_fil[k] - base + 28] = _dev(filled[k].reshape(-1), gpu_device)
    buf[a_lut - base: a_lut - base + 768] = _dev(luts.reshape(-1), gpu_device)
    buf[a_map - base: a_map - base + 4 * w] = _dev(cmap.view(np.uint8), gpu_device)
    sel3, sel1 = (C.c_uint32 * 3)(2, 1, 0), (C.c_uint32 * 1)(1)

    def hist(img, fil, r, h):
        return lib.mdemod_picture_histogram_device(C.byref(picture._SLOTS(*img)) if img else None, C.byref(picture._SLOTS(*fil)) if fil else None, r,
                                                   C.c_void_p(h), gpu_device, st)

    def render(img, fil, r, sel, planes, lut, cm, width, out, val):
        return lib.mdemod_picture_render_device(C.byref(picture._SLOTS(*img)) if img else None, C.byref(picture._SLOTS(*fil)) if fil else None, r, sel, planes,
                                                C.c_void_p(lut), C.c_void_p(cm), width, C.c_void_p(out), C.c_void_p(val), gpu_device, st)

    def refused(word, rc):
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text

    assert hist(a_img, a_fil, rows, a_hist) == 0 and render(a_img, a_fil, rows, sel3, 3, a_lut, a_map, w, a_out, a_val) == 0
    host = buf.cpu().numpy()
    assert np.array_equal(host[a_out - base: a_val - base].reshape(8 * rows, w, 3), want[(1, (2, 1, 0))][0])
    # rows = 0: the histogram is zeroed, the render has nothing to do and looks at no pointer
    assert hist(None, None, 0, a_hist) == 0 and render(None, None, 0, sel3, 3, 0, 0, w, 0, 0) == 0
    assert not buf[a_hist - base: a_hist - base + 3072].cpu().numpy().any()
    # only the selected slots are looked at
    assert render([0, a_img[1], 0], [0, a_fil[1], 0], rows, sel1, 1, a_lut, a_map, w, a_out, 0) == 0
    refused("needed", hist(a_img, a_fil, rows, 0))
    refused("needed", hist(None, a_fil, rows, a_hist))
    refused("mask of slot 1", hist(a_img, [a_fil[0], 0, a_fil[2]], rows, a_hist))
    refused("multiple of 4", hist(a_img, a_fil, rows, a_hist + 2))
    refused("multiples of 4", hist([a_img[0] + 1, a_img[1], a_img[2]], a_fil, rows, a_hist))
    refused("65536", hist(a_img, a_fil, 65537, a_hist))
    refused("intersect", hist(a_img, a_fil, rows, a_img[2] + n_img - 4))
    refused("intersect", hist(a_img, a_fil, rows, a_fil[0] - 3068))
    good = dict(img=a_img, fil=a_fil, r=rows, sel=sel3, planes=3, lut=a_lut, cm=a_map, width=w, out=a_out, val=a_val)
    for word, change in (("planes", dict(planes=2)), ("selection", dict(sel=None)), ("slot", dict(sel=(C.c_uint32 * 3)(0, 3, 1))), ("65536", dict(r=65537)),
                         ("width", dict(width=1566)), ("width", dict(width=0)), ("width", dict(width=8196)),
                         ("slot 2", dict(img=[a_img[0], a_img[1], 0])), ("slot 1", dict(fil=[a_fil[0], 0, a_fil[2]])), ("needed", dict(img=None)),
                         ("needed", dict(lut=0)), ("needed", dict(cm=0)), ("needed", dict(out=0)),
                         ("multiples of 4", dict(out=a_out + 2)), ("multiples of 4", dict(val=a_val + 1)), ("multiples of 4", dict(lut=a_lut + 1)),
                         ("multiples of 4", dict(cm=a_map + 2)), ("multiples of 4", dict(img=[a_img[0] + 2, a_img[1], a_img[2]])),
                         ("intersect", dict(out=a_img[0] + 4)), ("intersect", dict(out=a_map - 8 * rows * w * 3 + 4)), ("intersect", dict(val=a_lut)),
                         ("intersect", dict(val=a_out + 4)), ("intersect", dict(out=a_fil[1] - 8 * rows * w * 3 + 4))):
        refused(word, render(**{**good, **change}))
    for word, opts in (("altitude", dict(altitude_km=100)), ("scan angle", dict(scan_deg=170)), ("misses", dict(altitude_km=2000, scan_deg=100)),
                       ("clips", dict(clip_low=500)), ("piece_rows", dict(piece_rows=1 << 17))):
        with pytest.raises(_capi.MdemodError) as e:
            picture.compose(images, filled, (2, 1, 0), device=gpu_device, **opts)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        picture.compose(images, filled, (2, 1), device=gpu_device)
    assert "planes" in e.value.detail
    torch.cuda.synchronize(gpu_device)


# ---------------------------------------------------------------------------------------------------------------- pieces
def test_compose_host_in_pieces_equals_one_batch(gpu_device):
    """mdemod_picture_compose_host in pieces of 1 strip row, of 2, and in one: the same bytes, the model's bytes, and what the
    device-tensor path gives."""
    from meteor_demod_amd import picture
    rows = 5
    images, filled = PU.pixels(rows, 21), PU.masks("mixed", rows, 6)
    for select, opts in (((2, 1, 0), dict()), ((1,), dict(altitude_km=820, scan_deg=20, clip_low=100, clip_high=0)), ((0, 0, 2), dict(rectify=0, stretch=0))):
        model = picture.model_host(images, filled, select, **opts)
        whole = picture.compose(images, filled, select, device=gpu_device, **opts)
        one = picture.compose(images, filled, select, device=gpu_device, piece_rows=1, **opts)
        two = picture.compose(images, filled, select, device=gpu_device, piece_rows=2, **opts)
        tens = picture.compose([_dev(x, gpu_device) for x in images], [_dev(x, gpu_device) for x in filled], select, **opts)
        print(f"select {select}, {opts}: {whole.pixels.shape}, limits {whole.limits}, {100 * whole.valid_share:.1f} % valid")
        for got in (whole, one, two, tens):
            assert np.array_equal(got.pixels, model.pixels) and np.array_equal(got.valid, model.valid) and got.limits == model.limits


# --------------------------------------------------------------------------------------------------------------- streams
def test_sent_picture_to_composite(gpu_device):
    """image_util.picture through the sender, the image layer on the device and image_to_picture: the composite is the utility
    applied to the image layer's own result."""
    from meteor_demod_amd import image, picture
    rows = 2
    pic = I.picture(5, rows)
    vcdu, _, _ = I.mux(I.picture_packets(pic, 60))
    res = image.vcdu_to_image(_dev(vcdu, gpu_device))
    assert res.summary["rows"] == rows and all(res.filled[a].all() for a in (64, 65, 66))
    images, filled = [res.images[a] for a in (64, 65, 66)], [res.filled[a] for a in (64, 65, 66)]
    for composite, select, opts in (("auto", (2, 1, 0), dict()), ("123", (0, 1, 2), dict(rectify=0)), ("2", (1,), dict(altitude_km=900, scan_deg=114))):
        got = picture.image_to_picture(res, composite=composite, device=gpu_device, **opts)
        want, _, lim = PU.compose(images, filled, select, cmap=picture.column_map(**opts), **opts)
        want = want if len(select) == 3 else want[:, :, 0]
        print(f"composite {composite} {opts}: {got.pixels.shape}, limits {got.limits}, bytes {got.pixels.min()} .. {got.pixels.max()}")
        assert got.select == select and got.limits == lim and np.array_equal(got.pixels, want) and got.valid_share == 1.0
    # only the first two channels received strips: auto picks 221; only the first: none
    res.filled[66][:] = False
    two = picture.image_to_picture(res, composite="auto", device=gpu_device)
    assert two.select == (1, 1, 0) and np.array_equal(two.pixels[:, :, 0], two.pixels[:, :, 1])
    res.filled[65][:] = False
    assert picture.image_to_picture(res, composite="auto", device=gpu_device) is None


# ------------------------------------------------------------------------------------------------------------------- CLI
def _pnm(path, magic, planes):
    raw = path.read_bytes()
    m = re.match(magic + rb"\n(\d+) (\d+)\n255\n", raw)
    assert m, raw[:20]
    w, h = int(m.group(1)), int(m.group(2))
    assert len(raw) == m.end() + w * h * planes
    a = np.frombuffer(raw[m.end():], dtype=np.uint8)
    return a.reshape(h, w, 3) if planes == 3 else a.reshape(h, w)


def test_cli_rectify_and_composite(tmp_path, gpu_device):
    """--image --rectify --composite 321 on the recording of the picture: the three plain PGMs as before, three rectified ones and
    the PPM whose headers and bytes are the Python path's, the line; --composite alone is 1568 wide; auto; the refusals."""
    from conftest import ROOT
    from meteor_demod_amd import image, picture, rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    st, iq = I.recording()
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))

    def run(name, *flags):
        return subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), *flags, "-o", str(tmp_path / name), str(wav)], capture_output=True,
                              text=True, cwd=tmp_path, timeout=300)

    p = run("pass.s", "--cadu", "--image", "--rectify", "--composite", "321", "--altitude", "830", "--scan-angle", "108")
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    cadu = np.frombuffer((tmp_path / "pass.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    geo = dict(altitude_km=830, scan_deg=108)
    for k, a in enumerate((64, 65, 66)):
        assert np.array_equal(_pnm(tmp_path / f"pass_{a}.pgm", rb"P5", 1), res.images[a])
        want = picture.image_to_picture(res, composite=str(k + 1), device=gpu_device, **geo)
        got = _pnm(tmp_path / f"pass_{a}_rect.pgm", rb"P5", 1)
        assert got.shape == (8 * I.PIC_ROWS, want.width) and want.width > 1568 and np.array_equal(got, want.pixels)
    want = picture.image_to_picture(res, composite="321", device=gpu_device, **geo)
    got = _pnm(tmp_path / "pass_321.ppm", rb"P6", 3)
    assert np.array_equal(got, want.pixels)
    m = re.fullmatch(r"(\S+)pass: composite 321: (\d+) x (\d+) rectified; stretch R (\d+) \.\. (\d+), G (\d+) \.\. (\d+), B (\d+) \.\. (\d+); ([\d.]+) % of pixels valid",
                     p.stdout.strip().splitlines()[-1])
    assert m, p.stdout
    assert [int(m.group(k)) for k in range(2, 10)] == [want.width, 8 * I.PIC_ROWS] + [x for lim in want.limits for x in lim] and float(m.group(10)) == 100.0
    # --composite without --rectify: 1568 wide, stretched; auto picks 321 here; with --apids 64,65,68 the first two: 221
    q = run("flat.s", "--image", "--composite", "auto")
    assert q.returncode == 0, q.stderr
    flat = picture.image_to_picture(res, composite="321", device=gpu_device, rectify=0)
    assert np.array_equal(_pnm(tmp_path / "flat_321.ppm", rb"P6", 3), flat.pixels) and flat.width == 1568 and "composite 321: 1568 x 8;" in q.stdout
    assert not list(tmp_path.glob("flat*_rect.pgm"))
    q = run("two.s", "--image", "--composite", "auto", "--apids", "64,65,68")
    assert q.returncode == 0 and "composite 221" in q.stdout and (tmp_path / "two_221.ppm").exists()
    q = run("none.s", "--image", "--composite", "auto", "--apids", "64,68,69")
    assert q.returncode == 0 and "no composite" in q.stdout and not list(tmp_path.glob("none*.ppm"))
    for flags, word in ((("--rectify",), "only with --image"), (("--composite", "321"), "only with --image"), (("--image", "--altitude", "800"), "only with --rectify"),
                        (("--image", "--scan-angle", "100"), "only with --rectify"), (("--image", "--composite", "421"), "1 .. 3"),
                        (("--image", "--composite", "32"), "three digits"), (("--image", "--rectify", "--altitude", "100"), "altitude"),
                        (("--image", "--rectify", "--scan-angle", "131"), "scan angle"), (("--image", "--rectify", "--altitude", "2000"), "misses the Earth")):
        r = run("no.s", *flags)
        assert r.returncode == 1 and word in r.stderr and not (tmp_path / "no.s").exists(), (flags, r.stderr)
