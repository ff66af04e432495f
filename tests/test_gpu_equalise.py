"""GPU tests of the equalise layer (include/meteor_demod_amd_equalise.h): GPU bytes equal the host model's bytes, for the public
workspace (tables and counts) and for the output, over the sizes, pictures, masks and layouts of tests/equalise_ref.py with clips 100,
300 and 25 600 and amounts 0, 128 and 256.  Every case runs with its inputs inside garbage and canaries around the workspace and the
output, and everything but those two must come back as it was.  Then: in place against out of place, the two entries one after the
other against the joint one, the argument checks, the host entry and its summary, the Python entries, and the C host's --equalise.
Every GPU step runs once; every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import equalise_ref as R

pytestmark = pytest.mark.gpu

CLIPS = (100, 300, 25600)
AMOUNTS = (0, 128, 256)
GUARD = 64


def _stream(gpu_device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)


def _up4(n):
    return (n + 3) & ~3


class Arena:
    """One device buffer of garbage with the picture, the mask, the workspace and the output in it, GUARD bytes between them; the
    picture stands at 4 (not 16) bytes."""

    def __init__(self, pic, valid, need, gpu_device, seed=1, slack=0):
        import torch
        rng = np.random.default_rng(seed)
        self.pic_off = GUARD + 4
        self.valid_off = _up4(self.pic_off + pic.size) + GUARD + 1                    # (the mask needs no alignment)
        self.work_off = _up4(self.valid_off + (valid.size if valid is not None else 0)) + GUARD
        self.work_len = need + slack
        self.out_off = _up4(self.work_off + self.work_len) + GUARD
        total = _up4(self.out_off + pic.size) + GUARD
        self.host = rng.integers(0, 256, total, dtype=np.uint8)
        self.host[self.pic_off: self.pic_off + pic.size] = pic.ravel()
        if valid is not None:
            self.host[self.valid_off: self.valid_off + valid.size] = valid.ravel()
        self.pic, self.valid, self.need = pic, valid, need
        self.dev = torch.from_numpy(self.host.copy()).to(f"cuda:{gpu_device}")
        self.base = self.dev.data_ptr()
        assert self.base % 16 == 0

    def ptr(self, off):
        return C.c_void_p(self.base + off)

    @property
    def P(self):
        return self.ptr(self.pic_off)

    @property
    def V(self):
        return self.ptr(self.valid_off) if self.valid is not None else None

    @property
    def W(self):
        return self.ptr(self.work_off)

    @property
    def O(self):
        return self.ptr(self.out_off)

    def back(self, written):
        """The buffer from the device; everything outside the ranges `written` [(offset, bytes)] must be as it was."""
        got = self.dev.cpu().numpy()
        same = got == self.host
        for off, n in written:
            same[off: off + n] = True
        assert same.all(), f"{int((~same).sum())} bytes outside the outputs changed, the first at {int(np.argmin(same))}"
        return got


def _dims(pic):
    return (pic.shape[1], pic.shape[0], 1 if pic.ndim == 2 else pic.shape[2])


def _run(pic, valid, opts, gpu_device, inplace=False, split=False):
    """(workspace bytes, output) of the device entries on an arena; the canaries and the inputs checked."""
    from meteor_demod_amd import equalise as E
    from meteor_demod_amd._capi import check
    w, h, planes = _dims(pic)
    need = E.workspace(w, h, planes, opts)
    a = Arena(pic, valid, need, gpu_device, slack=8)
    out = a.P if inplace else a.O
    st = _stream(gpu_device)
    if split:
        check(E.lib().mdemod_equalise_tables_device(a.P, a.V, w, h, planes, C.byref(opts), a.W, need, gpu_device, st), "tables")
        check(E.lib().mdemod_equalise_apply_device(a.P, a.V, w, h, planes, C.byref(opts), a.W, out, gpu_device, st), "apply")
    else:
        check(E.lib().mdemod_equalise_device(a.P, a.V, w, h, planes, C.byref(opts), a.W, need, out, gpu_device, st), "both")
    out_off = a.pic_off if inplace else a.out_off
    got = a.back([(a.work_off, need), (out_off, pic.size)])
    return got[a.work_off: a.work_off + need], got[out_off: out_off + pic.size].reshape(pic.shape)


def _cases():
    i = 0
    for kind in R.PICTURES:
        for mask in R.MASKS:
            for planes, mode in R.LAYOUTS:
                yield kind, mask, planes, mode, CLIPS[i % 3], AMOUNTS[(i // 3 + i) % 3]
                i += 1


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}t{s[2]}")
def test_gpu_bytes_equal_model_bytes(size, gpu_device):
    from meteor_demod_amd import equalise as E
    w, h, tile = size
    n = bad_work = bad_out = empty = changed = 0
    pairs = set()
    for kind, mask, planes, mode, clip, amount in _cases():
        pic = R.picture_of(kind, w, h, planes)
        valid, step = R.mask_of(mask, kind, w, h, tile)
        opts = E.options(tile=tile, clip=clip / 100.0, amount=amount / 256.0, mode=mode, valid_step=step)
        work, out = _run(pic, valid, opts, gpu_device)
        want_work = E.model_workspace(pic, valid, opts)[: len(work)]
        want_out = E.model_apply(pic, valid, tile=tile, clip=clip / 100.0, amount=amount / 256.0, mode=mode, valid_step=step)
        dw, do = int((work != want_work).sum()), int((out != want_out).sum())
        if dw or do:
            print(f"{size} {kind} {mask} planes {planes} mode {mode} clip {clip} amount {amount}: {dw} bytes of the workspace and {do} of the output differ")
        bad_work += dw; bad_out += do
        tab, count = E._split(work, *E.geometry(w, h, planes, opts))
        if mask == "nothing":
            assert not count.any() and np.array_equal(out, pic)
        if kind == "one" and mask in ("none", "half", "gaps"):
            assert (count == 1).all()
        n += 1; empty += int((count == 0).sum()); changed += int((out != pic).sum())
        pairs.add((clip, amount))
    print(f"{size}: {n} cases, {len(pairs)} (clip, amount) pairs, {empty} empty tiles, {changed} bytes changed; differing: workspace {bad_work}, output {bad_out}")
    assert n == 75 and len(pairs) == 9 and empty > 0 and changed > 0
    assert bad_work == 0 and bad_out == 0


@pytest.mark.parametrize("size", [(39, 23, 16), (300, 203, 64)], ids=lambda s: f"{s[0]}x{s[1]}t{s[2]}")
def test_in_place_and_split_entries(size, gpu_device):
    """In place equals out of place, and the two entries one after the other equal the joint one."""
    from meteor_demod_amd import equalise as E
    w, h, tile = size
    for planes, mode in R.LAYOUTS:
        pic = R.picture_of("noise", w, h, planes)
        valid, step = R.mask_of("gaps", "noise", w, h, tile)
        opts = E.options(tile=tile, clip=3.0, amount=0.75, mode=mode)
        want = E.model_apply(pic, valid, tile=tile, clip=3.0, amount=0.75, mode=mode)
        results = {name: _run(pic, valid, opts, gpu_device, **kw) for name, kw in (("out of place", {}), ("in place", dict(inplace=True)), ("split", dict(split=True)),
                                                                                     ("split in place", dict(split=True, inplace=True)))}
        for name, (work, out) in results.items():
            print(f"{size} planes {planes} mode {mode} {name}: {int((out != want).sum())} bytes differ from the model, {int((out != pic).sum())} from the picture")
            assert np.array_equal(out, want) and np.array_equal(work, results["out of place"][0])


def test_argument_checks_leave_everything_untouched(gpu_device):
    from meteor_demod_amd import _capi, equalise as E
    w, h, planes, tile = 40, 24, 3, 16
    pic = R.picture_of("noise", w, h, planes)
    valid, _ = R.mask_of("half", "noise", w, h, tile)
    good = E.options(tile=tile)
    need = E.workspace(w, h, planes, good)
    a = Arena(pic, valid, need, gpu_device)
    st, lib, d = _stream(gpu_device), E.lib(), gpu_device
    n = 0

    def refused(word, rc):
        nonlocal n
        assert rc == _capi.MDEMOD_ERR_PARAM and word in _capi.last_error(), (word, rc, _capi.last_error())
        n += 1

    def both(word, *args_opts, **kw):
        """The same bad value through all three device entries."""
        o = kw.get("o", good)
        ww, hh, pp = kw.get("w", w), kw.get("h", h), kw.get("planes", planes)
        refused(word, lib.mdemod_equalise_tables_device(a.P, a.V, ww, hh, pp, C.byref(o), a.W, need, d, st))
        refused(word, lib.mdemod_equalise_apply_device(a.P, a.V, ww, hh, pp, C.byref(o), a.W, a.O, d, st))
        refused(word, lib.mdemod_equalise_device(a.P, a.V, ww, hh, pp, C.byref(o), a.W, need, a.O, d, st))
    both("width", w=0); both("width", w=8193); both("height", h=0); both("height", h=16385); both("planes", planes=2); both("planes", planes=0)
    for word, kw in (("tile", dict(tile=8)), ("tile", dict(tile=20)), ("tile", dict(tile=520)), ("clip_percent", dict(clip=0.99)), ("clip_percent", dict(clip=256.01)),
                     ("amount", dict(amount=1.01)), ("mode", dict(mode=2)), ("valid_step", dict(valid_step=2)), ("valid_step", dict(valid_step=0))):
        both(word, o=E.options(**{**dict(tile=tile), **kw}))
    O = C.byref(good)
    refused("picture is needed", lib.mdemod_equalise_tables_device(None, a.V, w, h, planes, O, a.W, need, d, st))
    refused("workspace is needed", lib.mdemod_equalise_tables_device(a.P, a.V, w, h, planes, O, None, need, d, st))
    refused("workspace is needed", lib.mdemod_equalise_apply_device(a.P, a.V, w, h, planes, O, None, a.O, d, st))
    refused("output is needed", lib.mdemod_equalise_apply_device(a.P, a.V, w, h, planes, O, a.W, None, d, st))
    refused("output is needed", lib.mdemod_equalise_device(a.P, a.V, w, h, planes, O, a.W, need, None, d, st))
    refused(f"needs {need} bytes", lib.mdemod_equalise_tables_device(a.P, a.V, w, h, planes, O, a.W, need - 1, d, st))
    refused(f"needs {need} bytes", lib.mdemod_equalise_device(a.P, a.V, w, h, planes, O, a.W, 0, a.O, d, st))
    refused("multiples of 4", lib.mdemod_equalise_tables_device(a.ptr(a.pic_off + 1), a.V, w, h - 1, planes, O, a.W, need, d, st))
    refused("multiples of 4", lib.mdemod_equalise_tables_device(a.P, a.V, w, h, planes, O, a.ptr(a.work_off + 2), need, d, st))
    refused("multiples of 4", lib.mdemod_equalise_apply_device(a.P, a.V, w, h, planes, O, a.W, a.ptr(a.out_off + 1), d, st))
    refused("intersect", lib.mdemod_equalise_tables_device(a.P, a.V, w, h, planes, O, a.ptr(a.pic_off + 8), need, d, st))
    refused("intersect", lib.mdemod_equalise_tables_device(a.P, a.ptr(a.work_off + 5), w, h, planes, O, a.W, need, d, st))
    refused("intersect", lib.mdemod_equalise_apply_device(a.P, a.V, w, h, planes, O, a.W, a.ptr(a.pic_off + 4), d, st))
    refused("intersect", lib.mdemod_equalise_apply_device(a.P, a.V, w, h, planes, O, a.W, a.ptr(a.work_off + 4), d, st))
    refused("intersect", lib.mdemod_equalise_device(a.P, a.V, w, h, planes, O, a.W, need, a.ptr(a.valid_off - 1 - 40), d, st))
    refused("intersect", lib.mdemod_equalise_device(a.P, a.ptr(a.pic_off + 40), w, h - 1, planes, O, a.W, need, a.O, d, st))
    import torch
    torch.cuda.synchronize(gpu_device)
    a.back([])
    print(f"{n} refusals, every byte of the {a.host.size} as it was")
    assert n == 3 * 15 + 16
    # ... and the entries work on these very buffers
    assert lib.mdemod_equalise_device(a.P, a.V, w, h, planes, O, a.W, need, a.O, d, st) == 0
    got = a.back([(a.work_off, need), (a.out_off, pic.size)])
    assert np.array_equal(got[a.out_off: a.out_off + pic.size].reshape(pic.shape), E.model_apply(pic, valid, tile=tile))


def test_host_entry_and_summary(gpu_device):
    from meteor_demod_amd import _capi, equalise as E
    for (w, h, tile), (planes, mode), mask in (((300, 203, 64), (3, 1), "gaps"), ((39, 23, 16), (1, 1), "step8"), ((1030, 67, 512), (3, 0), "none"), ((40, 24, 16), (3, 1), "nothing")):
        pic = R.picture_of("noise", w, h, planes)
        valid, step = R.mask_of(mask, "noise", w, h, tile)
        opts = E.options(tile=tile, clip=2.5, amount=0.9, mode=mode, valid_step=step)
        out, s = E.apply_host(pic, valid, opts, device=gpu_device)
        want = E.model_apply(pic, valid, tile=tile, clip=2.5, amount=0.9, mode=mode, valid_step=step)
        tab, count = E.model_tables(pic, valid, tile=tile, clip=2.5, amount=0.9, mode=mode, valid_step=step)
        print(f"{w} x {h} x {planes} mode {mode} {mask}: {s.nx} x {s.ny} tiles, {s.channels} channels, {s.empty_tiles} empty; {int((out != want).sum())} bytes differ")
        assert (s.channels, s.ny, s.nx) == count.shape and s.empty_tiles == int((count[0] == 0).sum())
        assert np.array_equal(out, want)
        if mask == "gaps":
            assert 0 < s.empty_tiles < s.nx * s.ny
        if mask == "nothing":
            assert s.empty_tiles == s.nx * s.ny and np.array_equal(out, pic)
    with pytest.raises(_capi.MdemodError) as e:
        E.apply_host(pic, None, E.options(tile=12), device=gpu_device)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "tile" in e.value.detail
    assert E.lib().mdemod_equalise_host(None, None, None, 4, 4, 1, None, gpu_device) == _capi.MDEMOD_ERR_PARAM and "picture is needed" in _capi.last_error()


def test_python_entries(gpu_device):
    import torch
    from meteor_demod_amd import equalise as E
    for planes, mode in ((1, "luma"), (3, "luma"), (3, "planes")):
        pic = R.picture_of("ramp", 300, 203, planes)
        valid, _ = R.mask_of("half", "ramp", 300, 203, 64)
        kw = dict(tile=64, clip=4.0, amount=0.5, mode=mode)
        want = E.model_apply(pic, valid, **kw)
        a = E.apply(pic, valid, device=gpu_device, **kw)
        t_in = torch.from_numpy(pic).to(f"cuda:{gpu_device}")
        t = E.apply(t_in, torch.from_numpy(valid).to(f"cuda:{gpu_device}"), **kw)
        tab, count = E.tables(pic, valid, device=gpu_device, **kw)
        mtab, mcount = E.model_tables(pic, valid, **kw)
        print(f"planes {planes} {mode}: array {int((a != want).sum())}, tensor {int((t.cpu().numpy() != want).sum())} bytes differ; tables {tab.shape}, "
              f"{int((tab != mtab).sum())} bytes and {int((count != mcount).sum())} counts differ")
        assert isinstance(a, np.ndarray) and a.shape == pic.shape and np.array_equal(a, want) and not np.shares_memory(a, pic)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.shape == t_in.shape and np.array_equal(t.cpu().numpy(), want) and np.array_equal(t_in.cpu().numpy(), pic)
        assert np.array_equal(tab, mtab) and np.array_equal(count, mcount)
    # the defaults: tile 128, clip 3, all of it, luminance, no mask
    pic = R.picture_of("noise", 300, 203, 3)
    assert np.array_equal(E.apply(pic, device=gpu_device), E.model_apply(pic))
    with pytest.raises(ValueError):
        E.apply(pic, mode="chroma")
    with pytest.raises(ValueError):
        E.apply(pic, np.zeros((5, 5), np.uint8))


# ------------------------------------------------------------------------------------------------------------------- CLI
def _pnm(path, magic, planes):
    raw = path.read_bytes()
    m = re.match(magic + rb"\n(\d+) (\d+)\n255\n", raw)
    assert m, raw[:20]
    w, h = int(m.group(1)), int(m.group(2))
    assert len(raw) == m.end() + w * h * planes
    a = np.frombuffer(raw[m.end():], dtype=np.uint8)
    return a.reshape(h, w, 3) if planes == 3 else a.reshape(h, w)


def test_cli_equalise(tmp_path, gpu_device):
    """--image --rectify --composite 321 --equalise 2.5 --equalise-tile 64 --equalise-amount 75 on the recording of the picture
    layer's CLI test: the channel pictures are as decoded, the written _rect and composite files equal the Python path's
    picture.compose (through image_to_picture) followed by equalise.apply under the picture's own mask at valid_step 8, and every
    derived picture has its line."""
    import frames_util as U
    import image_util as I
    from conftest import ROOT
    from meteor_demod_amd import equalise as E, image, picture, rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    st, iq = I.recording()
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    p = subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), "--cadu", "--image", "--rectify", "--composite", "321", "--equalise", "2.5", "--equalise-tile", "64",
                        "--equalise-amount", "75", "-o", str(tmp_path / "pass.s"), str(wav)], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    cadu = np.frombuffer((tmp_path / "pass.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    kw = dict(tile=64, clip=2.5, amount=0.75, valid_step=8)
    assert E.options(**kw).amount == 192 and int(2.56 * 75 + 0.5) == 192
    names = []
    for k, apid in enumerate((64, 65, 66)):
        assert np.array_equal(_pnm(tmp_path / f"pass_{apid}.pgm", rb"P5", 1), res.images[apid])
        pic = picture.image_to_picture(res, composite=str(k + 1), device=gpu_device)
        want = E.apply(pic.pixels, pic.valid, device=gpu_device, **kw)
        got = _pnm(tmp_path / f"pass_{apid}_rect.pgm", rb"P5", 1)
        print(f"pass_{apid}_rect.pgm: {got.shape}, {int((got != want).sum())} bytes differ, {int((got != pic.pixels).sum())} changed by the step")
        assert np.array_equal(got, want) and not np.array_equal(got, pic.pixels)
        names.append((f"pass_{apid}_rect.pgm", got.shape))
    pic = picture.image_to_picture(res, composite="321", device=gpu_device)
    want = E.apply(pic.pixels, pic.valid, device=gpu_device, **kw)
    got = _pnm(tmp_path / "pass_321.ppm", rb"P6", 3)
    print(f"pass_321.ppm: {got.shape}, {int((got != want).sum())} bytes differ, {int((got != pic.pixels).sum())} changed by the step")
    assert np.array_equal(got, want) and not np.array_equal(got, pic.pixels)
    names.append(("pass_321.ppm", got.shape))
    lines = [l for l in p.stdout.splitlines() if ": equalised: " in l]
    assert len(lines) == 4
    for (name, shape), line in zip(names, lines):
        nx, ny = max(1, (shape[1] + 32) // 64), max(1, (shape[0] + 32) // 64)
        m = re.fullmatch(r"(\S*)" + re.escape(name) + rf": equalised: tile 64, clip 2\.5, {nx} x {ny} tiles, (\d+) empty", line)
        assert m, line
        assert int(m.group(2)) == 0
