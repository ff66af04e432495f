"""GPU tests of the JPEG encoder (include/meteor_demod_amd_jpeg.h): the file of the kernels against the file of the host model, byte for
byte, over the sizes, qualities and restart intervals of the CPU round trip and on flat, noisy and checkered pictures; the entropy
stage alone on the crafted coefficients of jpeg_cases.py, with more than 8 segments, a short last segment and more segments than one
pass of the offset scan covers; canaries around every buffer; an output one byte short; the argument checks; the host entry; the
Python entry on a tensor and on an array; the C host's --jpeg.  Every GPU step runs once; every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

import jpeg_cases as K
import jpeg_ref as R
import map_util as MU
from test_gpu_map import _dev, _pnm, _stream_handle

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ file against model
@pytest.mark.parametrize("width,height", K.SIZES)
def test_file_equals_the_model(width, height, gpu_device):
    from meteor_demod_amd import jpeg as J
    bad = sizes = 0
    for planes in (1, 3):
        pic = K.picture(width, height, planes)
        d = _dev(pic, gpu_device)
        for quality in K.QUALITIES:
            for ri in K.INTERVALS:
                want, got = J.model_encode(pic, quality, ri), J.encode_tensor(d, quality, ri)
                bad += got != want
                sizes += len(got)
    print(f"{width} x {height}: 24 files, {sizes} bytes, {bad} differ from the model")
    assert bad == 0


@pytest.mark.parametrize("kind", ["flat", "noise", "checker"])
def test_hard_pictures_equal_the_model(kind, gpu_device):
    """A flat picture (segments of a few bits), uniform noise at quality 100 (stuffing, long codes), a 0 / 255 checkerboard of period 1
    (the largest coefficients); 300 x 203 reaches past one strip of the transform and ends in part blocks both ways."""
    from meteor_demod_amd import jpeg as J
    w, h = 300, 203
    rng = np.random.default_rng(3)
    for planes in (1, 3):
        shape = (h, w, 3) if planes == 3 else (h, w)
        if kind == "flat":
            pic = np.full(shape, 201, np.uint8)
        elif kind == "noise":
            pic = rng.integers(0, 256, shape, dtype=np.uint8)
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            pic = (((xx + yy) & 1) * 255).astype(np.uint8)
            pic = np.stack([pic, 255 - pic, pic], axis=2) if planes == 3 else pic
        for quality, ri in ((100, 0), (50, 7), (100, 64)):
            want, got = J.model_encode(pic, quality, ri), J.encode_tensor(_dev(pic, gpu_device), quality, ri)
            print(f"{kind} x {planes}, quality {quality}, Ri {ri}: {len(want)} bytes, {want.count(bytes([255, 0]))} stuffed, largest level {int(np.abs(J.model_coefficients(pic, quality)).max())}")
            assert got == want


# ------------------------------------------------------------------------------------------------------------ entropy stage
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("ri", [1, 2, 32, 64])
def test_entropy_on_crafted_coefficients(planes, ri, gpu_device):
    """The crafted coefficients (runs, no EOB, zero blocks, DC edges, largest magnitudes, values out of range, 32 stuffed bytes and
    more in a segment, a segment that ends on an FF).  Ri 1 and 2: far more than 8 segments (the markers wrap); Ri 32 and 64: a short
    last segment (105 and 35 MCUs)."""
    from meteor_demod_amd import jpeg as J
    coef = K.crafted_for(planes)
    n_mcus = len(coef) // planes
    want = J.model_entropy(coef, planes, ri)
    got = J.entropy(_dev(coef, gpu_device), planes, ri)
    segs = -(-n_mcus // ri)
    print(f"{planes} planes, Ri {ri}: {segs} segments, the last of {n_mcus - (segs - 1) * ri} MCUs, {len(want)} bytes")
    assert got == want and (ri > 2 or segs > 8) and (ri < 32 or n_mcus % ri)
    assert np.array_equal(R.entropy_only(got, n_mcus, planes, ri, K.dht_of(J)), K.clamped(coef))


def test_entropy_more_segments_than_one_pass_of_the_scan(gpu_device):
    """Ri 1 on the blocks of a 2048 x 512 grey picture: 16 384 segments, 16 passes of the offset scan's 1024 threads, and on 3075
    colour MCUs, whose last pass is part full."""
    from meteor_demod_amd import jpeg as J
    rng = np.random.default_rng(11)
    for planes, n_mcus in ((1, 256 * 64), (3, 3075)):
        coef = (rng.integers(-1024, 1024, (n_mcus * planes, 64)) * (rng.random((n_mcus * planes, 64)) < 0.08)).astype(np.int16)
        coef[:: 7] = 0
        want = J.model_entropy(coef, planes, 1)
        got = J.entropy(_dev(coef, gpu_device), planes, 1)
        print(f"{n_mcus} segments x {planes}: {len(want)} bytes")
        assert got == want


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """Picture, output, workspace and result inside canaries at shifts 0, 4 and 1000 (the workspace at the next multiple of 16): the
    canaries survive, the picture is only read, the file is the model's.  With out_room one byte short the result names the bytes
    needed and no byte of the output changes."""
    import torch
    from meteor_demod_amd import _capi, jpeg as J
    w, h, quality, ri = 100, 70, 90, 5
    pad, wpad = 64 + shift, 64 + (shift + 15) // 16 * 16
    st = _stream_handle(gpu_device)
    for planes in (1, 3):
        pic = K.picture(w, h, planes, 1)
        want = J.model_encode(pic, quality, ri)
        need_work = J.workspace(w, h, planes, ri)
        for room in (len(want), len(want) + 100, len(want) - 1):
            dev = f"cuda:{gpu_device}"
            src = torch.full((pad + pic.size + 64,), 0x5A, dtype=torch.uint8, device=dev)
            out = torch.full((pad + room + 64,), 0xC3, dtype=torch.uint8, device=dev)
            work = torch.full((wpad + need_work + 64,), 0x3C, dtype=torch.uint8, device=dev)
            res = torch.full((8 + 16 + 8,), 0x77, dtype=torch.uint8, device=dev)
            src[pad: pad + pic.size] = _dev(pic.reshape(-1), gpu_device)
            before = src.cpu().numpy()
            assert J.lib().mdemod_jpeg_encode_device(C.c_void_p(src.data_ptr() + pad), w, h, planes, quality, ri, C.c_void_p(out.data_ptr() + pad), room,
                                                     C.c_void_p(res.data_ptr() + 8), C.c_void_p(work.data_ptr() + wpad), need_work, gpu_device, st) == 0
            n = C.c_uint64()
            rc = J.lib().mdemod_jpeg_result(C.c_void_p(res.data_ptr() + 8), C.byref(n), gpu_device, st)
            o, k, r = out.cpu().numpy(), work.cpu().numpy(), res.cpu().numpy()
            print(f"shift {shift}, {planes} planes, room {room} of {len(want)}: rc {rc}, {n.value} bytes; '{_capi.last_error()}'")
            assert n.value == len(want) and np.array_equal(src.cpu().numpy(), before)
            assert (o[:pad] == 0xC3).all() and (o[pad + room:] == 0xC3).all() and (k[:wpad] == 0x3C).all() and (k[wpad + need_work:] == 0x3C).all()
            assert (r[:8] == 0x77).all() and (r[24:] == 0x77).all()
            if room >= len(want):
                assert rc == 0 and o[pad: pad + len(want)].tobytes() == want and (o[pad + len(want): pad + room] == 0xC3).all()
            else:
                assert rc == _capi.MDEMOD_ERR_OVERFLOW and str(len(want)) in _capi.last_error() and (o == 0xC3).all()


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    """Every refusal of both device entries with its text, and nothing written."""
    import torch
    from meteor_demod_amd import _capi, jpeg as J
    lib, st = J.lib(), _stream_handle(gpu_device)
    w, h = 40, 24
    pic = K.picture(w, h, 3)
    area, room, need = pic.size, J.bound(w, h, 3), J.workspace(w, h, 3)
    need16 = (need + 15) // 16 * 16
    buf = torch.full((area + 16 + room + need16 + 16 + 64,), 0xEE, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    assert base % 16 == 0
    a_pic = base
    a_work = base + (area + 15) // 16 * 16
    a_res = a_work + need16
    a_out = a_res + 16
    buf[:area] = _dev(pic.reshape(-1), gpu_device)
    before = buf.cpu().numpy()

    def enc(p=a_pic, width=w, height=h, planes=3, quality=90, ri=0, out=a_out, out_room=room, res=a_res, work=a_work, work_bytes=need):
        return lib.mdemod_jpeg_encode_device(C.c_void_p(p), width, height, planes, quality, ri, C.c_void_p(out), out_room, C.c_void_p(res), C.c_void_p(work), work_bytes,
                                             gpu_device, st)
    for word, change in (("planes", dict(planes=2)), ("width", dict(width=0)), ("width", dict(width=8193)), ("height", dict(height=0)), ("height", dict(height=16385)),
                         ("quality", dict(quality=0)), ("quality", dict(quality=101)), ("restart interval", dict(ri=65)), ("input is needed", dict(p=0)),
                         ("output is needed", dict(out=0)), ("result is needed", dict(res=0)), ("workspace is needed", dict(work=0)),
                         ("workspace needs", dict(work_bytes=need - 1)), ("multiples of 16", dict(work=a_work + 8)), ("multiple of 8", dict(res=a_res + 4)),
                         ("intersect", dict(out=a_pic + area - 1)), ("intersect", dict(work=a_pic)), ("intersect", dict(out=a_work + need - 1)), ("intersect", dict(res=a_out + 8)),
                         ("intersect", dict(res=a_work)), ("intersect", dict(res=a_pic + area - 8))):
        rc = enc(**change)
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text
    coef = torch.zeros((6, 64), dtype=torch.int16, device=f"cuda:{gpu_device}")
    a_coef = coef.data_ptr()

    def ent(p=a_coef, n_mcus=2, planes=3, ri=0, out=a_out, out_room=room, res=a_res, work=a_work, work_bytes=need):
        return lib.mdemod_jpeg_entropy_device(C.c_void_p(p), n_mcus, planes, ri, C.c_void_p(out), out_room, C.c_void_p(res), C.c_void_p(work), work_bytes, gpu_device, st)
    for word, change in (("planes", dict(planes=0)), ("MCUs", dict(n_mcus=0)), ("MCUs", dict(n_mcus=(1 << 21) + 1)), ("restart interval", dict(ri=65)), ("input is needed", dict(p=0)),
                         ("multiples of 16", dict(p=a_coef + 2)), ("workspace needs", dict(work_bytes=8)), ("intersect", dict(out=a_coef, out_room=16)),
                         ("result is needed", dict(res=0))):
        rc = ent(**change)
        text = _capi.last_error()
        print(f"entropy, {word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text
    assert lib.mdemod_jpeg_result(None, None, gpu_device, st) == _capi.MDEMOD_ERR_PARAM
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(buf.cpu().numpy(), before) and not coef.cpu().numpy().any()         # nothing was written
    # and the same buffers, unchanged arguments: the model's file, twice the same
    assert enc() == 0
    n = C.c_uint64()
    assert lib.mdemod_jpeg_result(C.c_void_p(a_res), C.byref(n), gpu_device, st) == 0
    want = J.model_encode(pic, 90, 0)
    o = a_out - base
    assert buf.cpu().numpy()[o: o + n.value].tobytes() == want


# ------------------------------------------------------------------------------------------------------- host and python
def test_host_entry_and_python(gpu_device, monkeypatch):
    """mdemod_jpeg_encode_host equals the device entry and the model; ``encode`` gives the same bytes for a tensor on the GPU and a
    numpy array; ``write`` writes them; the tensor entry grows its buffer for a picture that codes to more than twice its size."""
    from meteor_demod_amd import _capi, jpeg as J
    for (w, h), planes, quality, ri in (((333, 77), 3, 90, 0), ((64, 64), 1, 50, 3), ((1, 1), 3, 100, 64)):
        pic = K.picture(w, h, planes, 2)
        want = J.model_encode(pic, quality, ri)
        host, tensor = J.encode(pic, quality, ri, device=gpu_device), J.encode(_dev(pic, gpu_device), quality, ri)
        print(f"{w} x {h} x {planes}: {len(want)} bytes")
        assert host == want and tensor == want
    noise = np.random.default_rng(4).integers(0, 256, (8, 8), dtype=np.uint8)
    monkeypatch.setattr(J, "_first_room", lambda *a: 100)                             # (less than the head: the second attempt)
    assert J.encode_tensor(_dev(noise, gpu_device), 100, 1) == J.model_encode(noise, 100, 1)
    monkeypatch.undo()
    with pytest.raises(_capi.MdemodError) as e:
        J.encode_tensor(_dev(pic, gpu_device), 100, 64, out_room=len(want) - 1)
    assert e.value.code == _capi.MDEMOD_ERR_OVERFLOW and str(len(want)) in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        J.encode(pic, 0, device=gpu_device)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "quality" in e.value.detail


def test_write(tmp_path, gpu_device):
    from meteor_demod_amd import jpeg as J
    pic = K.picture(50, 30, 3, 3)
    n = J.write(tmp_path / "p.jpg", _dev(pic, gpu_device), 75)
    data = (tmp_path / "p.jpg").read_bytes()
    assert n == len(data) and data == J.model_encode(pic, 75) and R.decode(data).pixels.shape == (30, 50, 3)


# ------------------------------------------------------------------------------------------------------------------- CLI
def _psnr_floor(J, quality, planes):
    """What any picture keeps at this quality: no level is further than Q / 2 from its coefficient, the transform is orthonormal, so a
    component's mean square error is at most mean(Q^2) / 4; R, G and B take Y's error and that of the chrominance through the JFIF
    equations (1.402^2 + 0.344^2 + 0.714^2 + 1.772^2 over the three of them); the roundings of the colour transform there and
    back are at most 0.5 (1 + 0.7) + 0.5 = 1.35 on a sample, added to the root of the mean square; clamping to 0 .. 255 only brings
    a sample nearer."""
    q = J.model_tables(quality)[0].astype(float)
    mse = (q[0] ** 2).mean() / 4
    if planes == 3:
        mse += (q[1] ** 2).mean() / 4 * (1.402 ** 2 + 0.344136 ** 2 + 0.714136 ** 2 + 1.772 ** 2) / 3
    return 20 * np.log10(255.0 / (np.sqrt(mse) + 1.35))


def test_cli_jpeg(tmp_path, gpu_device):
    """The one-row recording through --image --rectify --composite 321 --map --graticule 5 with --jpeg 90 and without: every .pgm /
    .ppm of the plain run has its .jpg in the other, which is the model's file of those pixels and decodes (jpeg_ref) to them within
    the floor above; the world files are the same bytes; the plain run writes no .jpg, its map is the Python pipeline's, and its
    stdout is the other's without the JPEG lines."""
    import frames_util as U
    from conftest import GOLDEN, ROOT
    from meteor_demod_amd import image, jpeg as J, map as M, rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    tle = GOLDEN / "map_tle.txt"
    _, iq = MU.recording()
    dirs = [tmp_path / "jpeg", tmp_path / "plain"]
    for d in dirs:
        d.mkdir()
        (d / "one.wav").write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    common = ("--cadu", "--image", "--rectify", "--composite", "321", "--map", str(tle), "--map-scale", "60", "--scan-angle", "108", "--graticule", "5")

    def run(cwd, *flags):
        return subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), *common, *flags, "-o", "one.s", "one.wav"], capture_output=True, text=True, cwd=cwd, timeout=300)
    p, q = run(dirs[0], "--jpeg", "90"), run(dirs[1])
    assert p.returncode == 0, p.stderr
    assert q.returncode == 0, q.stderr
    print(p.stdout)
    plain = sorted(f.name for f in dirs[1].iterdir() if f.suffix in (".pgm", ".ppm"))
    assert len(plain) >= 9 and not list(dirs[1].glob("*.jpg")) and not list(dirs[0].glob("*.p?m"))
    assert {"one_64.pgm", "one_64_rect.pgm", "one_321.ppm", "one_321_map.ppm", "one_321_map_overlay.ppm"} <= set(plain)
    bytes_in = bytes_out = 0
    for name in plain:
        planes = 3 if name.endswith(".ppm") else 1
        pixels = _pnm(dirs[1] / name, rb"P6" if planes == 3 else rb"P5", planes)
        data = (dirs[0] / (name[:-4] + ".jpg")).read_bytes()
        back = R.decode(data)
        got, floor = K.psnr(back.pixels, pixels), _psnr_floor(J, 90, planes)
        print(f"{name}: {pixels.shape}, {len(data)} bytes, {got:.2f} dB (floor {floor:.2f})")
        assert data == J.model_encode(pixels, 90, 0) and back.restart_interval == 32 and got >= floor
        assert f"{name[:-4]}.jpg: JPEG quality 90: {pixels.shape[1]} x {pixels.shape[0]} x {planes}, {len(data)} bytes of {pixels.size}\n" in p.stdout
        bytes_in, bytes_out = bytes_in + pixels.size, bytes_out + len(data)
    assert p.stdout.splitlines()[-1] == f"--jpeg 90: {len(plain)} files, {bytes_in} bytes of pictures in, {bytes_out} bytes of JPEG out"
    for f in dirs[1].glob("*.wld"):
        assert (dirs[0] / f.name).read_bytes() == f.read_bytes()
    assert [l for l in p.stdout.splitlines() if "JPEG quality" not in l and not l.startswith("--jpeg")] == q.stdout.splitlines()
    # the plain run is what it was: the map is the Python pipeline's
    cadu = np.frombuffer((dirs[1] / "one.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    one = M.image_to_map(res, tle.read_text(), composite="321", device=gpu_device, px_per_deg=60, scan_deg=108)
    assert np.array_equal(_pnm(dirs[1] / "one_321_map.ppm", rb"P6", 3), one.pixels)
    # refusals before anything is demodulated
    for flags, word in ((("--jpeg", "0"), "1 .. 100"), (("--jpeg", "x"), "1 .. 100")):
        r = run(dirs[1], *flags)
        assert r.returncode == 1 and word in r.stderr
    r = subprocess.run([str(cli_exe), "-q", "-B", "--jpeg", "90", "one.wav"], capture_output=True, text=True, cwd=dirs[1], timeout=60)
    assert r.returncode == 1 and "only with --image" in r.stderr
