"""GPU tests of the PNG encoder (include/meteor_demod_amd_png.h): the file of the kernels against the file of the host model, byte for
byte, over the sizes of the CPU round trip, with and without a mask, and on flat, noisy and checkered pictures; the deflate stage
alone on the crafted arrays of png_cases.py and on more segments than one pass of the offset scan holds; canaries around every
buffer; an output one byte short; the argument checks; the host entry; the Python entry on tensors, on arrays and on another
stream; the command line in a fresh process.  Every GPU step runs once; every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

import png_cases as K
import png_ref as R
from conftest import ROOT
from test_gpu_map import _stream_handle

pytestmark = pytest.mark.gpu

FILTERS = (0, 4, 5)
SEGMENTS = (1, 32)


def _dev(a, gpu_device):
    """A copy of the array on the GPU (the shared fixtures are read-only)."""
    import torch
    return torch.from_numpy(np.array(a)).to(f"cuda:{gpu_device}")


def _scan_threads() -> int:
    """The segments one pass of the offset scan holds: the scan kernel's own constant."""
    return int(re.search(r"#define ENC_SCAN_THREADS\s+(\d+)", (ROOT / "meteor_demod_amd" / "csrc" / "encoder_device.h").read_text()).group(1))


# ------------------------------------------------------------------------------------------------------ file against model
@pytest.mark.parametrize("width,height", K.SIZES)
def test_file_equals_the_model(width, height, gpu_device):
    from meteor_demod_amd import png as P
    bad = sizes = files = 0
    for planes in (1, 3):
        pic = K.picture(width, height, planes)
        d = _dev(pic, gpu_device)
        for valid in (None, K.mask(width, height)):
            v = _dev(valid, gpu_device) if valid is not None else None
            for filt in FILTERS:
                for segment in SEGMENTS:
                    want, got = P.model_encode(pic, valid, filt, segment), P.encode_tensor(d, v, filt, segment)
                    bad += got != want
                    sizes += len(got)
                    files += 1
    print(f"{width} x {height}: {files} files, {sizes} bytes, {bad} differ from the model")
    assert bad == 0 and files == 24


@pytest.mark.parametrize("kind", ["flat", "noise", "checker"])
def test_hard_pictures_equal_the_model(kind, gpu_device):
    """A flat picture (runs across whole segments), uniform noise (stored segments), a 0 / 255 checkerboard of period 1; 1100 x 67
    reaches past one tile of the filter and, with a mask, past two segments of 32 KiB."""
    from meteor_demod_amd import png as P
    w, h = 1100, 67
    rng = np.random.default_rng(3)
    valid = K.mask(w, h, 2)
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
        for filt, segment, va in ((5, 0, None), (0, 7, valid), (3, 32, None), (1, 1, valid), (2, 2, None)):
            want = P.model_encode(pic, va, filt, segment)
            got = P.encode_tensor(_dev(pic, gpu_device), _dev(va, gpu_device) if va is not None else None, filt, segment)
            print(f"{kind} x {planes}, filter {filt}, segment {segment}, mask {va is not None}: {len(want)} bytes of {pic.size}")
            assert got == want


# ------------------------------------------------------------------------------------------------------------ deflate stage
@pytest.mark.parametrize("name", sorted(K.crafted()))
def test_deflate_on_crafted_bytes(name, gpu_device):
    """The crafted arrays (every run length around the rule's edges, a run across a segment start, equal bytes, all values once, noise,
    a last segment of one byte, counts that force the length limit of both codes): the chunks are the model's and inflate back."""
    from meteor_demod_amd import png as P
    data, segment = K.crafted()[name]
    want = P.model_deflate(data, segment)
    got = P.deflate(_dev(data, gpu_device), segment)
    print(f"{name}: {data.size} bytes, segment {segment} KiB: {len(want)} bytes of chunks")
    assert got == want
    assert R.inflate_raw(b"".join(b for _, b in R.chunks(got, 0))) == data.tobytes()


def test_more_segments_than_one_pass_of_the_scan(gpu_device):
    """Segments of 1 KiB: two full passes of the offset scan and a part of a third on bytes alone, and a picture whose filtered
    stream is a little more than one pass."""
    from meteor_demod_amd import png as P
    n_scan = _scan_threads()
    rng = np.random.default_rng(11)
    n = (2 * n_scan + 37) * 1024 + 5
    data = (rng.integers(0, 256, n) * (rng.random(n) < 0.3)).astype(np.uint8)
    data[5 * 1024: 9 * 1024] = rng.integers(0, 256, 4 * 1024)                          # some stored segments among them
    want = P.model_deflate(data, 1)
    got = P.deflate(_dev(data, gpu_device), 1)
    print(f"{-(-n // 1024)} segments, {n_scan} a pass: {len(want)} bytes")
    assert -(-n // 1024) > 2 * n_scan and got == want
    h = n_scan // 2 + 3
    pic, valid = K.picture(700, h, 3, 5), K.mask(700, h, 5)
    want = P.model_encode(pic, valid, 5, 1)
    got = P.encode_tensor(_dev(pic, gpu_device), _dev(valid, gpu_device), 5, 1)
    print(f"700 x {h} x 4: {-(-h * 2801 // 1024)} segments, {len(want)} bytes")
    assert h * 2801 > n_scan * 1024 and got == want


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """Picture, mask, output, workspace and result inside canaries at shifts 0, 4 and 1000 (the workspace at the next multiple of 16),
    the inputs inside garbage: the canaries survive, the inputs are only read, the file is the model's.  With out_room one byte short
    the result names the bytes needed and no byte of the output changes."""
    import torch
    from meteor_demod_amd import _capi, png as P
    w, h, filt, segment = 100, 70, 5, 2
    pad, wpad = 64 + shift, 64 + (shift + 15) // 16 * 16
    st = _stream_handle(gpu_device)
    dev = f"cuda:{gpu_device}"
    for planes in (1, 3):
        pic, valid = K.picture(w, h, planes, 1), K.mask(w, h, 1)
        want = P.model_encode(pic, valid, filt, segment)
        need_work = P.workspace(w, h, planes, True, segment)
        for room in (len(want), len(want) + 100, len(want) - 1):
            src = torch.full((pad + pic.size + 64,), 0x5A, dtype=torch.uint8, device=dev)
            msk = torch.full((pad + valid.size + 64,), 0xA5, dtype=torch.uint8, device=dev)
            out = torch.full((pad + room + 64,), 0xC3, dtype=torch.uint8, device=dev)
            work = torch.full((wpad + need_work + 64,), 0x3C, dtype=torch.uint8, device=dev)
            res = torch.full((8 + 16 + 8,), 0x77, dtype=torch.uint8, device=dev)
            src[pad: pad + pic.size] = _dev(pic.reshape(-1), gpu_device)
            msk[pad: pad + valid.size] = _dev(valid.reshape(-1), gpu_device)
            before, mbefore = src.cpu().numpy(), msk.cpu().numpy()
            assert P.lib().mdemod_png_encode_device(C.c_void_p(src.data_ptr() + pad), C.c_void_p(msk.data_ptr() + pad), w, h, planes, filt, segment,
                                                    C.c_void_p(out.data_ptr() + pad), room, C.c_void_p(res.data_ptr() + 8), C.c_void_p(work.data_ptr() + wpad), need_work,
                                                    gpu_device, st) == 0
            n = C.c_uint64()
            rc = P.lib().mdemod_png_result(C.c_void_p(res.data_ptr() + 8), C.byref(n), gpu_device, st)
            o, k, r = out.cpu().numpy(), work.cpu().numpy(), res.cpu().numpy()
            print(f"shift {shift}, {planes} planes, room {room} of {len(want)}: rc {rc}, {n.value} bytes; '{_capi.last_error()}'")
            assert n.value == len(want) and np.array_equal(src.cpu().numpy(), before) and np.array_equal(msk.cpu().numpy(), mbefore)
            assert (o[:pad] == 0xC3).all() and (o[pad + room:] == 0xC3).all() and (k[:wpad] == 0x3C).all() and (k[wpad + need_work:] == 0x3C).all()
            assert (r[:8] == 0x77).all() and (r[24:] == 0x77).all()
            if room >= len(want):
                assert rc == 0 and o[pad: pad + len(want)].tobytes() == want and (o[pad + len(want): pad + room] == 0xC3).all()
            else:
                assert rc == _capi.MDEMOD_ERR_OVERFLOW and str(len(want)) in _capi.last_error() and (o == 0xC3).all()


def test_guard_regions_of_the_deflate_stage(gpu_device):
    """The bytes of the deflate entry inside garbage, its output and workspace inside canaries; a short last segment of 3 bytes (the
    loads of whole words stop before it)."""
    import torch
    from meteor_demod_amd import _capi, png as P
    st = _stream_handle(gpu_device)
    dev = f"cuda:{gpu_device}"
    data = (np.arange(2 * 1024 + 3) % 7).astype(np.uint8)
    want = P.model_deflate(data, 1)
    need_work = int(P.lib().mdemod_png_deflate_workspace(data.size, 1))
    for room in (len(want), len(want) - 1):
        src = torch.full((64 + data.size + 64,), 0x5A, dtype=torch.uint8, device=dev)
        out = torch.full((68 + room + 64,), 0xC3, dtype=torch.uint8, device=dev)
        work = torch.full((64 + need_work + 64,), 0x3C, dtype=torch.uint8, device=dev)
        res = torch.zeros(2, dtype=torch.int64, device=dev)
        src[64: 64 + data.size] = _dev(data, gpu_device)
        assert P.lib().mdemod_png_deflate_device(C.c_void_p(src.data_ptr() + 64), data.size, 1, C.c_void_p(out.data_ptr() + 68), room, C.c_void_p(res.data_ptr()),
                                                 C.c_void_p(work.data_ptr() + 64), need_work, gpu_device, st) == 0
        n = C.c_uint64()
        rc = P.lib().mdemod_png_result(C.c_void_p(res.data_ptr()), C.byref(n), gpu_device, st)
        o, k = out.cpu().numpy(), work.cpu().numpy()
        print(f"room {room} of {len(want)}: rc {rc}, {n.value} bytes")
        assert n.value == len(want) and (o[:68] == 0xC3).all() and (o[68 + room:] == 0xC3).all() and (k[:64] == 0x3C).all() and (k[64 + need_work:] == 0x3C).all()
        assert (rc == 0 and o[68: 68 + room].tobytes() == want) if room >= len(want) else (rc == _capi.MDEMOD_ERR_OVERFLOW and (o == 0xC3).all())


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    """Every refusal of both device entries with its text, and nothing written."""
    import torch
    from meteor_demod_amd import _capi, png as P
    lib, st = P.lib(), _stream_handle(gpu_device)
    w, h = 40, 24
    pic, valid = K.picture(w, h, 3), K.mask(w, h)
    area, room, need = pic.size, P.bound(w, h, 3, True), P.workspace(w, h, 3, True)
    need16, area16 = (need + 15) // 16 * 16, (area + 15) // 16 * 16
    buf = torch.full((area16 + 1024 + room + need16 + 16 + 64,), 0xEE, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    assert base % 16 == 0
    a_pic, a_valid = base, base + area16
    a_work = a_valid + 1024
    a_res = a_work + need16
    a_out = a_res + 16
    buf[:area] = _dev(pic.reshape(-1), gpu_device)
    buf[area16: area16 + valid.size] = _dev(valid.reshape(-1), gpu_device)
    before = buf.cpu().numpy()

    def enc(p=a_pic, v=a_valid, width=w, height=h, planes=3, filt=5, segment=0, out=a_out, out_room=room, res=a_res, work=a_work, work_bytes=need):
        return lib.mdemod_png_encode_device(C.c_void_p(p), C.c_void_p(v), width, height, planes, filt, segment, C.c_void_p(out), out_room, C.c_void_p(res), C.c_void_p(work),
                                            work_bytes, gpu_device, st)
    for word, change in (("planes", dict(planes=2)), ("width", dict(width=0)), ("width", dict(width=8193)), ("height", dict(height=0)), ("height", dict(height=16385)),
                         ("filter", dict(filt=6)), ("segment", dict(segment=33)), ("input is needed", dict(p=0)),
                         ("output is needed", dict(out=0)), ("result is needed", dict(res=0)), ("workspace is needed", dict(work=0)),
                         ("workspace needs", dict(work_bytes=need - 1)), ("multiples of 16", dict(work=a_work + 8)), ("multiple of 8", dict(res=a_res + 4)),
                         ("intersect", dict(out=a_pic + area - 1)), ("intersect", dict(work=a_pic)), ("intersect", dict(out=a_work + need - 1)), ("intersect", dict(res=a_out + 8)),
                         ("intersect", dict(res=a_work)), ("intersect", dict(res=a_pic + area - 8)), ("intersect", dict(out=a_valid + 8, out_room=8)),
                         ("intersect", dict(v=a_work + 16))):
        rc = enc(**change)
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text
    data = torch.zeros(4096, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    a_data = data.data_ptr()

    def dfl(p=a_data, n_bytes=4096, segment=1, out=a_out, out_room=room, res=a_res, work=a_work, work_bytes=need):
        return lib.mdemod_png_deflate_device(C.c_void_p(p), n_bytes, segment, C.c_void_p(out), out_room, C.c_void_p(res), C.c_void_p(work), work_bytes, gpu_device, st)
    for word, change in (("bytes are outside", dict(n_bytes=0)), ("bytes are outside", dict(n_bytes=(1 << 30) + 1)), ("segment", dict(segment=33)), ("input is needed", dict(p=0)),
                         ("multiples of 16", dict(p=a_data + 4)), ("workspace needs", dict(work_bytes=8)), ("intersect", dict(out=a_data, out_room=16)),
                         ("result is needed", dict(res=0))):
        rc = dfl(**change)
        text = _capi.last_error()
        print(f"deflate, {word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text
    assert lib.mdemod_png_result(None, None, gpu_device, st) == _capi.MDEMOD_ERR_PARAM
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(buf.cpu().numpy(), before) and not data.cpu().numpy().any()         # nothing was written
    # and the same buffers, unchanged arguments: the model's file; a second call reusing them all: the same again
    want = P.model_encode(pic, valid)
    for _ in range(2):
        assert enc() == 0
        n = C.c_uint64()
        assert lib.mdemod_png_result(C.c_void_p(a_res), C.byref(n), gpu_device, st) == 0
        o = a_out - base
        assert buf.cpu().numpy()[o: o + n.value].tobytes() == want


# ------------------------------------------------------------------------------------------------------- host and python
def test_host_entry_and_python(gpu_device):
    """mdemod_png_encode_host equals the device entry and the model; ``encode`` gives the same bytes for tensors on the GPU and for numpy
    arrays, on the current stream when that is not the default one; too small a room and a bad filter raise with code and text."""
    import torch
    from meteor_demod_amd import _capi, png as P
    for (w, h), planes, masked, filt, segment in (((333, 77), 3, True, 5, 0), ((64, 64), 1, False, 4, 3), ((1, 1), 3, True, 0, 32), ((1500, 9), 1, True, 5, 1)):
        pic = K.picture(w, h, planes, 2)
        valid = K.mask(w, h, 2) if masked else None
        want = P.model_encode(pic, valid, filt, segment)
        host = P.encode(pic, valid, filt, segment, device=gpu_device)
        tensor = P.encode(_dev(pic, gpu_device), _dev(valid, gpu_device) if masked else None, filt, segment)
        side = torch.cuda.Stream(device=gpu_device)
        with torch.cuda.stream(side):
            d, v = _dev(pic, gpu_device), _dev(valid, gpu_device) if masked else None
            streamed = P.encode(d, v, filt, segment)
        side.synchronize()
        print(f"{w} x {h} x {planes}, mask {masked}: {len(want)} bytes")
        assert host == want and tensor == want and streamed == want
        back = R.read(host)
        assert np.array_equal(back["pixels"].reshape(pic.shape), pic) and (not masked or np.array_equal(back["alpha"], np.where(valid != 0, 255, 0)))
    with pytest.raises(_capi.MdemodError) as e:
        P.encode_tensor(_dev(pic, gpu_device), None, 5, 1, out_room=len(P.model_encode(pic, None, 5, 1)) - 1)
    assert e.value.code == _capi.MDEMOD_ERR_OVERFLOW and str(len(P.model_encode(pic, None, 5, 1))) in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        P.encode(pic, None, 6, device=gpu_device)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "filter" in e.value.detail
    with pytest.raises(ValueError):
        P.encode_tensor(_dev(pic, gpu_device), _dev(np.zeros((2, 2), np.uint8), gpu_device))


def test_write(tmp_path, gpu_device):
    from meteor_demod_amd import png as P
    pic, valid = K.picture(50, 30, 3, 3), K.mask(50, 30, 3)
    n = P.write(tmp_path / "p.png", _dev(pic, gpu_device), _dev(valid, gpu_device), 4, 2)
    data = (tmp_path / "p.png").read_bytes()
    assert n == len(data) and data == P.model_encode(pic, valid, 4, 2) and np.array_equal(R.read(data)["pixels"], pic)
    m = P.write(tmp_path / "q.png", pic[:, :, 1], device=gpu_device)
    assert m == len((tmp_path / "q.png").read_bytes()) and np.array_equal(R.read((tmp_path / "q.png").read_bytes())["pixels"][:, :, 0], pic[:, :, 1])


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_command_line(tmp_path, gpu_device):
    """python -m meteor_demod_amd.png in a fresh child process on a .ppm and a .pgm: a .png beside each, the model's bytes, the
    pixels back, a line per file; with --valid-from-black the pixels whose planes are all 0 are transparent and the others opaque."""
    from meteor_demod_amd import png as P
    pic = np.array(K.picture(90, 40, 3, 4))
    pic[5:9, 7:30] = 0
    pic[20, 3] = (0, 0, 9)                                                            # one plane is not black: valid
    grey = np.ascontiguousarray(pic[:, :, 0])
    for flags in ((), ("--valid-from-black",)):
        d = tmp_path / ("masked" if flags else "plain")
        d.mkdir()
        (d / "one_321_map.ppm").write_bytes(b"P6\n90 40\n255\n" + pic.tobytes())
        (d / "one_64.pgm").write_bytes(b"P5\n90 40\n255\n" + grey.tobytes())
        (d / "one_321_map.wld").write_text("0.1\n")
        p = subprocess.run([sys.executable, "-m", "meteor_demod_amd.png", "--device", str(gpu_device), *flags, str(d / "one_321_map.ppm"), str(d / "one_64.pgm")],
                           capture_output=True, text=True, cwd=str(ROOT), timeout=120)
        assert p.returncode == 0, p.stderr
        print(p.stdout)
        lines = p.stdout.splitlines()
        assert len(lines) == 2 and sorted(f.name for f in d.iterdir()) == ["one_321_map.png", "one_321_map.ppm", "one_321_map.wld", "one_64.pgm", "one_64.png"]
        for name, px, line in (("one_321_map.png", pic, lines[0]), ("one_64.png", grey, lines[1])):
            data = (d / name).read_bytes()
            valid = (px.reshape(40, 90, -1).max(axis=2) != 0).astype(np.uint8) if flags else None
            back = R.read(data)
            assert data == P.model_encode(px, valid) and np.array_equal(back["pixels"].reshape(px.shape), px)
            assert (back["alpha"] is None) if not flags else (np.array_equal(back["alpha"], valid * 255) and back["alpha"][6, 8] == 0)
            assert not flags or back["alpha"][20, 3] == (255 if px.ndim == 3 else 0)
            assert line == f"{d / name}: 90 x 40 x {px.shape[2] if px.ndim == 3 else 1}, {len(data)} bytes out of {px.size} bytes in"
    r = subprocess.run([sys.executable, "-m", "meteor_demod_amd.png", str(tmp_path / "missing.ppm")], capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode != 0
