"""CPU tests of the front end (include/meteor_demod_amd_frontend.h): the filter design, the refusals, the exports and guards of
the new entries, the C host linked without them, and a sanitizer fuzz of mdemod_fe_design.  No GPU is touched."""
from __future__ import annotations

import ctypes as C
import json
import math
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
HEADER = ROOT / "include" / "meteor_demod_amd_frontend.h"
FE_SOURCES = [CSRC / "frontend.hip", CSRC / "frontend_design.cpp"]


def _design(fs, d, symrate=72000, offset=300000.0, tpp=16, bps=16, offsets=None):
    from meteor_demod_amd import DemodConfig, FrontEndConfig, design_taps
    return design_taps(DemodConfig(samplerate=fs, symrate=symrate, bps=bps), FrontEndConfig(offset, d, tpp),
                       n_streams=len(offsets) if offsets else 1, offsets=offsets)


def _response_db(h, fs, freqs):
    n = np.arange(len(h))
    return 20 * np.log10(np.abs(np.exp(-2j * np.pi * np.outer(np.asarray(freqs) / fs, n)) @ h.astype(np.float64)))


@pytest.mark.parametrize("fs,d,symrate", [(2400000, 8, 72000), (2048000, 8, 72000), (3000000, 12, 80000), (10000000, 40, 72000),
                                          (1024000, 4, 72000)])
def test_design_passband_and_alias_rejection(fs, d, symrate):
    """L = tpp D + 1, symmetric, sum 1; flat within 0.01 dB over +-0.8 symrate; >= 75 dB below every band that folds onto it."""
    h, _ = _design(fs, d, symrate)
    assert len(h) == 16 * d + 1 and h.dtype == np.float32
    assert np.array_equal(h, h[::-1])
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= 1e-6
    b = 0.8 * symrate
    f = np.linspace(-b, b, 801)
    assert _response_db(h, fs, f).min() >= -0.01
    fo = fs / d
    for k in range(1, d):
        assert -_response_db(h, fs, f + k * fo).max() >= 75.0, (k, fs, d)


def test_design_d1_and_phase_step():
    from meteor_demod_amd.frontend import phase_step
    h, step = _design(250000, 1, offset=0.0)
    assert h.tolist() == [1.0] and step == 0
    for fs, off in ((2400000, 300000.0), (2400000, -300000.0), (2500000, -0.37 * 2500000), (2000000, 312500.0), (2048000, 1.5)):
        _, step = _design(fs, 8, offset=off)
        want = int(np.int64(np.round(-off / fs * 2.0 ** 32))) & 0xFFFFFFFF   # (no exact halves among these)
        assert step == want == phase_step(off, fs), (fs, off)
    _, step = _design(2400000, 8, offsets=[-100000.0, 5.0])
    assert step == phase_step(-100000.0, 2400000)


@pytest.mark.parametrize("kw,word", [
    (dict(fs=2400000, d=7), "divide"),                                  # fs % D
    (dict(fs=2400000, d=16), "2.4"),                                    # 150 kS/s < 2.4 x 72k
    (dict(fs=2400000, d=8, offset=1200000.0), "offset"),                # |offset| >= fs / 2
    (dict(fs=2400000, d=8, offset=-1300000.0), "offset"),
    (dict(fs=2400000, d=8, offset=math.nan), "finite"),
    (dict(fs=2400000, d=8, offset=math.inf), "finite"),
    (dict(fs=2400000, d=8, offsets=[0.0, math.nan]), "finite"),
    (dict(fs=2400000, d=0), "decimation"),
    (dict(fs=25600000, d=129), "decimation"),
    (dict(fs=2400000, d=8, tpp=7), "taps_per_phase"),
    (dict(fs=2400000, d=8, tpp=33), "taps_per_phase"),
])
def test_design_refusals_name_the_setting(kw, word):
    from meteor_demod_amd import _capi
    with pytest.raises(_capi.MdemodError) as e:
        _design(**kw)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM
    assert word in e.value.detail, e.value.detail


def _header_entries():
    text = HEADER.read_text()
    return re.findall(r"^\s*(?:[\w ]+?\s*\*?\s*)\b(mdemod_fe_\w+)\s*\(", text, re.M)


def test_frontend_entries_exported_and_bound():
    """Every entry of the new header is exported by the library and typed in frontend.py's own table - and the main binding
    table is untouched (tests/test_host_logic.py pins it to the two older headers)."""
    from meteor_demod_amd import _capi, frontend
    names = _header_entries()
    assert len(names) == 10, names
    lib = frontend.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(frontend.SIGNATURES) == sorted(names)
    assert not any(n.startswith("mdemod_fe_") for n in _capi.SIGNATURES)
    assert "mdemod_fe" not in (ROOT / "include" / "meteor_demod_amd.h").read_text()


def test_frontend_int_entries_are_function_try_blocks():
    """No C++ exception crosses the boundary: every int entry of the new sources is `try { MDEMOD_API_ENTER ... } MDEMOD_API_CATCH`."""
    found = 0
    entries = set(_header_entries())
    for src in FE_SOURCES:
        text = src.read_text()
        for m in re.finditer(r"^(?:extern \"C\" )?int\n(mdemod_fe_\w+)\(", text, re.M):
            if m.group(1) not in entries:
                continue                                  # (internal helpers)
            found += 1
            body = text[m.end():]
            head = body[: body.index("{")]
            assert head.rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            end = body.index("\n}")                       # the function's last line: the handler
            assert body[end:].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 7, found


def test_fe_params_layout():
    from meteor_demod_amd.frontend import MdemodFeParams
    assert C.sizeof(MdemodFeParams) == 24


def _wav(path, fs, bps, samples: np.ndarray):
    import struct
    data = samples.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1 if bps != 32 else 3, 2, fs,
                                                                                    fs * 2 * bps // 8, 2 * bps // 8, bps)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(data)) + data)


def test_cli_without_frontend_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has no front end): it links, --help lists the new options, and
    --decimate 8 exits non-zero saying that the library has no front end - not "unrecognized option" - and writes nothing."""
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--offset" in h.stderr and "--decimate" in h.stderr
    wav = tmp_path / "in.wav"
    _wav(wav, 2400000, 16, np.zeros((16384, 2), dtype=np.int16))
    for extra in (["--decimate", "8"], ["--offset", "-300k"]):
        r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), *extra, str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0
        assert "no front end" in r.stderr and "unrecognized" not in r.stderr, r.stderr
        assert not (tmp_path / "out.s").exists()
        assert not list(tmp_path.glob("LRPT_*.s"))
    r = subprocess.run([str(exe), "-q", "--offset", "abc", str(wav)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "--offset" in r.stderr


@pytest.mark.timeout(300)
def test_design_fuzz_under_asan_ubsan(tmp_path):
    exe = tmp_path / "fuzz_fe_design"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_fe_design.cpp"), str(CSRC / "frontend_design.cpp"),
                        str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "30000", "7", "2.0"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["cases"] == 30000 and rep["accepted"] > 5000, rep
