"""The C host's --sun (include/meteor_demod_amd_sun.h) on the one-row recording with real stamps of map_util.recording(), once
with and once without the option: the channel pictures are the same files in both runs, and with --sun the _rect pictures, the
composite and the map are byte for byte what the Python chain makes of ``sun.correct``'s result; the line on stdout; the option
refusals, which need no GPU."""
from __future__ import annotations

import re
import subprocess

import numpy as np
import pytest

import map_util as MU
from conftest import GOLDEN, ROOT

CLI = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
TLE = GOLDEN / "map_tle.txt"


def _pnm(path, magic, planes):
    raw = path.read_bytes()
    m = re.match(magic + rb"\n(\d+) (\d+)\n255\n", raw)
    assert m, raw[:20]
    w, h = int(m.group(1)), int(m.group(2))
    assert len(raw) == m.end() + w * h * planes
    a = np.frombuffer(raw[m.end():], dtype=np.uint8)
    return a.reshape(h, w, 3) if planes == 3 else a.reshape(h, w)


@pytest.mark.gpu
def test_cli_sun(tmp_path, gpu_device):
    import frames_util as U
    from meteor_demod_amd import image, map as M, picture, rs, sun
    st, iq = MU.recording()
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))

    def run(name, *flags):
        return subprocess.run([str(CLI), "-q", "-B", "--device", str(gpu_device), "--cadu", "--image", "--rectify", "--composite", "321", "--map", str(TLE), "--map-scale", "60",
                               *flags, "-o", str(tmp_path / name), str(wav)], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    plain, p = run("plain.s"), run("pass.s", "--sun", "--sun-ref", "50", "--sun-limit", "80")
    assert plain.returncode == 0 and p.returncode == 0, plain.stderr + p.stderr
    print(p.stdout)
    assert ": sun: " not in plain.stdout
    cadu = np.frombuffer((tmp_path / "pass.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    cor = sun.correct(res, TLE.read_text(), device=gpu_device, ref_deg=50, limit_deg=80)
    assert cor.sun["slot_mask"] == 7 and list(cor.images) == [64, 65, 66]
    for k, apid in enumerate((64, 65, 66)):
        # the channel pictures stay as decoded: the same bytes in both runs
        assert (tmp_path / f"pass_{apid}.pgm").read_bytes() == (tmp_path / f"plain_{apid}.pgm").read_bytes()
        assert np.array_equal(_pnm(tmp_path / f"pass_{apid}.pgm", rb"P5", 1), res.images[apid]) and not np.array_equal(cor.images[apid], res.images[apid])
        want = picture.image_to_picture(cor, composite=str(k + 1), device=gpu_device)
        got = _pnm(tmp_path / f"pass_{apid}_rect.pgm", rb"P5", 1)
        print(f"pass_{apid}_rect.pgm: {got.shape}, {int((got != want.pixels).sum())} bytes differ from the Python chain, "
              f"{int((got != _pnm(tmp_path / f'plain_{apid}_rect.pgm', rb'P5', 1)).sum())} from the run without --sun")
        assert np.array_equal(got, want.pixels)
    want = picture.image_to_picture(cor, composite="321", device=gpu_device)
    got = _pnm(tmp_path / "pass_321.ppm", rb"P6", 3)
    assert np.array_equal(got, want.pixels)
    wmap = M.image_to_map(cor, TLE.read_text(), composite="321", device=gpu_device, px_per_deg=60)
    got = _pnm(tmp_path / "pass_321_map.ppm", rb"P6", 3)
    assert np.array_equal(got, wmap.pixels) and wmap.valid.any()
    assert (tmp_path / "pass_321_map.wld").read_text() == (tmp_path / "plain_321_map.wld").read_text()
    # the step does something: the corrected channel pictures differ, and a derived picture of the other run is not this run's
    # (the stretch takes a common factor out again, but not the limit's clipping at 255)
    differ = [name for name in ("321.ppm", "321_map.ppm", "64_rect.pgm") if (tmp_path / f"pass_{name}").read_bytes() != (tmp_path / f"plain_{name}").read_bytes()]
    print(f"files that differ between the runs: {differ}")
    lines = [l for l in p.stdout.splitlines() if ": sun: " in l]
    assert len(lines) == 1
    m = re.fullmatch(r"(\S*)pass: sun: zenith ([\d.]+) \.\. ([\d.]+) deg, reference 50, limit 80 \((\d+) of (\d+) nodes beyond it, (\d+) missing\); corrected: 64, 65, 66; "
                     r"([\d.]+) % of pixels saturated", lines[0])
    assert m, lines[0]
    s = cor.sun
    assert abs(float(m.group(2)) - s["zenith_min"]) < 0.006 and abs(float(m.group(3)) - s["zenith_max"]) < 0.006
    assert [int(m.group(k)) for k in (4, 5, 6)] == [s["at_limit"], s["nodes"], s["missing"]] and s["nodes"] == 2 * 99
    share = 100.0 * sum(s["saturated"]) / (3 * 8 * 1568)
    assert abs(float(m.group(7)) - share) < 0.0006
    # the line stands before the derived pictures' lines and after the image layer's
    out = p.stdout.splitlines()
    assert out.index(lines[0]) > next(i for i, l in enumerate(out) if "image packets" in l) and out.index(lines[0]) < next(i for i, l in enumerate(out) if ": map 321" in l)


@pytest.mark.parametrize("flags, word", [
    (("--image", "--sun"), "--sun: only with --map"),
    (("--sun", "--map", str(TLE)), "only with --image"),
    (("--sun",), "--sun: only with --image"),
    (("--image", "--map", str(TLE), "--sun-ref", "40"), "--sun-ref / --sun-limit: only with --sun"),
    (("--image", "--map", str(TLE), "--sun-limit", "80"), "--sun-ref / --sun-limit: only with --sun"),
    (("--image", "--map", str(TLE), "--sun", "--sun-ref", "81"), "--sun-ref: degrees of zenith angle, 0 .. 80"),
    (("--image", "--map", str(TLE), "--sun", "--sun-limit", "59"), "--sun-limit: degrees of zenith angle, 60 .. 89"),
    (("--image", "--map", str(TLE), "--sun", "--sun-limit", "x"), "--sun-limit: degrees of zenith angle, 60 .. 89"),
])
def test_cli_sun_refusals(tmp_path, flags, word):
    """One line on stderr, exit status 1, before any file is opened (no GPU is touched)."""
    p = subprocess.run([str(CLI), "-q", "-B", *flags, "-o", str(tmp_path / "no.s"), str(tmp_path / "none.wav")], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    print(p.returncode, p.stderr.strip())
    assert p.returncode == 1 and word in p.stderr and len(p.stderr.strip().splitlines()) == 1 and not list(tmp_path.iterdir())
