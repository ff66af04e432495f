"""CPU tests of the survey (include/meteor_demod_amd_survey.h): the detector on spectra made by numpy, the plan, the refusals, the
exports and guards of the new entries, the C host linked without them, and a sanitizer fuzz of mdemod_survey_plan and
mdemod_survey_detect.  No GPU is touched."""
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
HEADER = ROOT / "include" / "meteor_demod_amd_survey.h"
SURVEY_SOURCES = [CSRC / "survey.hip", CSRC / "survey_detect.cpp"]
FS, SYM, N, NFFT = 2400000, 72000, 1 << 21, 4096


# ------------------------------------------------------------------------------------------ the prototype's signals, in numpy
def _rrc(alpha, sps, span):
    t = np.arange(-span * sps, span * sps + 1) / sps
    h = np.zeros_like(t)
    for i, x in enumerate(t):
        if abs(x) < 1e-9:
            h[i] = 1 - alpha + 4 * alpha / np.pi
        elif abs(abs(4 * alpha * x) - 1) < 1e-9:
            h[i] = alpha / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / 4 / alpha) + (1 - 2 / np.pi) * np.cos(np.pi / 4 / alpha))
        else:
            h[i] = (np.sin(np.pi * x * (1 - alpha)) + 4 * alpha * x * np.cos(np.pi * x * (1 + alpha))) / (np.pi * x * (1 - (4 * alpha * x) ** 2))
    return h / np.sqrt((h ** 2).sum())


@pytest.fixture(scope="module")
def baseband():
    """Unit-power QPSK at 72 ksym/s, RRC 0.6, at 2.4 MS/s (x100 up, /3 down), 2^21 samples, at 0 Hz."""
    rng = np.random.default_rng(1)
    up, dec = 100, 3
    ns = N * dec // up + 40
    s = (rng.integers(0, 2, ns) * 2 - 1) + 1j * (rng.integers(0, 2, ns) * 2 - 1)
    z = np.zeros(ns * up, complex)
    z[::up] = s
    h = _rrc(0.6, up, 8)
    length = len(z) + len(h) - 1
    size = 1 << int(np.ceil(np.log2(length)))
    y = np.fft.ifft(np.fft.fft(z, size) * np.fft.fft(h, size))[:length][len(h) // 2::dec][:N]
    return y / np.sqrt((abs(y) ** 2).mean())


def _welch(x, nfft=NFFT, rows=1):
    """float64 Welch (Hann, no overlap), cast to f32: what the spectrum kernel computes."""
    m = len(x) // nfft
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)
    p = np.abs(np.fft.fftshift(np.fft.fft(x[: m * nfft].reshape(m, nfft) * w, axis=1), axes=1)) ** 2
    per = m // rows
    return np.array([p[r * per: (m if r == rows - 1 else (r + 1) * per)].mean(axis=0) for r in range(rows)]).astype(np.float32)


def _recording(baseband, f0, esn0_db, seed, others=True):
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    nv = (FS / SYM) / 10 ** (esn0_db / 10)
    x = baseband * np.exp(2j * np.pi * f0 / FS * t) + np.sqrt(nv / 2) * (rng.normal(size=N) + 1j * rng.normal(size=N))
    if others:
        x = x + np.exp(1j * (2 * np.pi * (-600000.0) / FS * t + 17000 / 2400 * np.sin(2 * np.pi * 2400 / FS * t)))
        x = x + 2.0 * np.exp(2j * np.pi * 700000.0 / FS * t) + 0.5            # a carrier of four times the power, and the DC spike
    return x


def _cfg(fs=FS, symrate=SYM, bps=16):
    from meteor_demod_amd import DemodConfig
    return DemodConfig(samplerate=fs, symrate=symrate, bps=bps)


# ---------------------------------------------------------------------------------------------------------------- detection
@pytest.mark.parametrize("f0", [301234.0, -873456.0, 1234.0])
def test_detect_finds_lrpt_the_carrier_and_the_fm_signal(f0, baseband):
    """The prototype's 15 cases (Es/N0 15, 9, 6, 3, 0 dB x three offsets), next to an FM signal of the same power, a carrier of
    four times the power and a DC spike: the LRPT candidate is among the hits within one bin; the carrier and the FM signal are
    hits too (detection does not confirm), and both are stronger than the LRPT hit at 0 dB."""
    from meteor_demod_amd import survey
    for k, esn0 in enumerate((15, 9, 6, 3, 0)):
        psd = _welch(_recording(baseband, f0, esn0, seed=100 + k))
        hits = survey.detect(_cfg(), psd)
        err = min(abs(h.coarse_offset_hz - f0) for h in hits)
        print(f"f0 {f0:+.0f} Es/N0 {esn0}: {[(round(h.coarse_offset_hz), round(h.psd_snr_db, 1)) for h in hits]}: error {err:.0f} Hz")
        assert err <= FS / NFFT, (f0, esn0, err)
        lrpt = min(hits, key=lambda h: abs(h.coarse_offset_hz - f0))
        assert abs(lrpt.psd_snr_db - esn0) <= 3.0 or abs(f0) < 50000          # (the DC spike sits inside the signal at +1 234 Hz)
        for f in (-600000.0, 700000.0):
            assert any(abs(h.coarse_offset_hz - f) <= 0.8 * SYM for h in hits), (f0, esn0, f)
        assert all(h.offset_hz == h.coarse_offset_hz and not h.confirmed and not h.refined and h.clock_quality == 0 for h in hits)
        assert [h.psd_snr_db for h in hits] == sorted((h.psd_snr_db for h in hits), reverse=True)
    carrier = next(h for h in hits if abs(h.coarse_offset_hz - 700000.0) <= 0.8 * SYM)
    assert carrier.psd_snr_db > lrpt.psd_snr_db                             # power alone picks the wrong thing


def test_detect_noise_alone_gives_no_hit():
    rng = np.random.default_rng(5)
    x = 4.0 * (rng.normal(size=N) + 1j * rng.normal(size=N))
    from meteor_demod_amd import survey
    psd = _welch(x)
    assert survey.detect(_cfg(), psd) == []
    loose = survey.detect(_cfg(), psd, min_snr_db=-60.0)
    print([round(h.psd_snr_db, 1) for h in loose])
    assert loose and max(h.psd_snr_db for h in loose) < -15.0                 # (about -20 dB over 2^21 samples)


def test_detect_drops_a_signal_at_the_band_edge(baseband):
    """1.16 MHz is closer to fs / 2 = 1.2 MHz than 0.8 symrate = 57.6 kHz: dropped; at 1.10 MHz it is a hit."""
    from meteor_demod_amd import survey
    for f0, found in ((1160000.0, False), (-1160000.0, False), (1100000.0, True)):
        hits = survey.detect(_cfg(), _welch(_recording(baseband, f0, 15, seed=9, others=False)))
        near = [h for h in hits if abs(h.coarse_offset_hz - f0) <= 0.8 * SYM]
        assert bool(near) == found, (f0, hits)
        assert all(abs(h.coarse_offset_hz) <= FS / 2 - 0.8 * SYM for h in hits)


def test_detect_best_row_and_max_candidates(baseband):
    """A signal that is there in the last quarter only: best_row is the last of four rows.  max_candidates limits the list."""
    from meteor_demod_amd import survey
    x = _recording(baseband, 301234.0, 15, seed=11)
    x[: 3 * N // 4] -= (baseband * np.exp(2j * np.pi * 301234.0 / FS * np.arange(N)))[: 3 * N // 4]
    hits = survey.detect(_cfg(), _welch(x, rows=4))
    lrpt = min(hits, key=lambda h: abs(h.coarse_offset_hz - 301234.0))
    assert abs(lrpt.coarse_offset_hz - 301234.0) <= FS / NFFT and lrpt.best_row == 3
    assert len(survey.detect(_cfg(), _welch(x, rows=4), max_candidates=2)) == 2
    assert survey.detect(_cfg(), np.zeros((2, 512), dtype=np.float32)) == []       # an empty spectrum: nothing, not an error


# --------------------------------------------------------------------------------------------------------- plan and refusals
def test_survey_plan_defaults():
    from meteor_demod_amd import survey_plan
    assert survey_plan(_cfg(2400000)) == (4096, 12)
    assert survey_plan(_cfg(10000000)) == (16384, 50)
    assert survey_plan(_cfg(230000)) == (512, 1)
    assert survey_plan(_cfg(2048000)) == (4096, 10)                 # 204 800 S/s >= 172 800
    assert survey_plan(_cfg(2400000, symrate=80000)) == (4096, 12)
    assert survey_plan(_cfg(100000000, symrate=72000))[0] == 16384               # clamped
    assert survey_plan(_cfg(2400000, symrate=1000000))[0] == 256                 # clamped


@pytest.mark.parametrize("kw,word", [
    (dict(cfg=dict(fs=172799)), "nothing to survey"),
    (dict(cfg=dict(fs=0)), "sample rate"),
    (dict(cfg=dict(symrate=0)), "symbol rate"),
    (dict(cfg=dict(bps=12)), "bits per sample"),
    (dict(shape=(1, 1000)), "fft_size"),
    (dict(shape=(1, 128)), "fft_size"),
    (dict(shape=(1, 32768)), "fft_size"),
    (dict(shape=(4097, 256)), "n_rows"),
    (dict(opts=dict(max_candidates=33)), "max_candidates"),
    (dict(opts=dict(min_snr_db=math.nan)), "min_snr_db"),
    (dict(opts=dict(min_snr_db=math.inf)), "min_snr_db"),
    (dict(opts=dict(fft_size=3000)), "fft_size"),
    (dict(opts=dict(n_rows=5000)), "n_rows"),
    (dict(opts=dict(decimation=200)), "decimation"),
    (dict(opts=dict(decimation=-3)), "decimation"),
    (dict(opts=dict(clock_threshold=-1.0)), "clock_threshold"),
    (dict(opts=dict(carrier_threshold=math.nan)), "carrier_threshold"),
    (dict(poison=math.nan), "not finite"),
    (dict(poison=math.inf), "not finite"),
])
def test_detect_refusals_name_the_setting(kw, word):
    from meteor_demod_amd import _capi, survey
    psd = np.ones(kw.get("shape", (1, 512)), dtype=np.float32)
    if "poison" in kw:
        psd[0, 77] = kw["poison"]
    with pytest.raises(_capi.MdemodError) as e:
        survey.detect(_cfg(**kw.get("cfg", {})), psd, **kw.get("opts", {}))
    assert e.value.code == _capi.MDEMOD_ERR_PARAM
    assert word in e.value.detail, e.value.detail


def test_plan_refusals_and_unknown_option():
    from meteor_demod_amd import _capi, survey, survey_plan
    for cfg, word in ((_cfg(100000), "nothing to survey"), (_cfg(-5), "sample rate"), (_cfg(bps=24), "bits per sample")):
        with pytest.raises(_capi.MdemodError) as e:
            survey_plan(cfg)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail
    with pytest.raises(TypeError):
        survey.detect(_cfg(), np.ones((1, 512), dtype=np.float32), min_snr=3)


# ------------------------------------------------------------------------------------------------------- exports and guards
def _header_entries():
    return re.findall(r"^\s*(?:int|void)\s+(mdemod_\w+)\s*\(", HEADER.read_text(), re.M)


def test_survey_entries_exported_and_bound():
    """Every entry of the new header is exported by the library and typed in survey.py's own table; the two older binding
    tables and headers are untouched."""
    from meteor_demod_amd import _capi, frontend, survey
    names = _header_entries()
    assert len(names) == 6, names
    lib = survey.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(survey.SIGNATURES) == sorted(names)
    assert not any("survey" in n or "spectrum" in n for n in list(_capi.SIGNATURES) + list(frontend.SIGNATURES))
    for h in ("meteor_demod_amd.h", "meteor_demod_amd_frontend.h"):
        assert "survey" not in (ROOT / "include" / h).read_text()
    import meteor_demod_amd
    for n in ("survey", "Hit", "survey_plan"):
        assert n in meteor_demod_amd.__all__ and hasattr(meteor_demod_amd, n)
    assert callable(survey.spectrum) and callable(survey.detect) and callable(survey.survey)


def test_survey_int_entries_are_function_try_blocks():
    """No C++ exception crosses the boundary: every int entry of the new sources is `try { MDEMOD_API_ENTER ... } MDEMOD_API_CATCH`."""
    found = 0
    entries = set(_header_entries())
    for src in SURVEY_SOURCES:
        text = src.read_text()
        for m in re.finditer(r"^(?:extern \"C\" )?int\n(mdemod_\w+)\(", text, re.M):
            if m.group(1) not in entries:
                continue                                  # (internal helpers)
            found += 1
            body = text[m.end():]
            head = body[: body.index("{")]
            assert head.rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            end = body.index("\n}")
            assert body[end:].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 5, found


def test_survey_struct_layouts():
    from meteor_demod_amd.survey import MdemodSurveyHit, MdemodSurveyOpts
    assert C.sizeof(MdemodSurveyOpts) == 32 and C.sizeof(MdemodSurveyHit) == 40
    assert MdemodSurveyOpts.min_snr_db.offset == 16 and MdemodSurveyHit.psd_snr_db.offset == 16 and MdemodSurveyHit.refined.offset == 36


def test_survey_host_code_is_hip_free_and_kernels_use_no_float_atomics():
    host = (CSRC / "survey_detect.cpp").read_text()
    assert not re.search(r"\bhip[A-Z_]|__global__|__device__|hip_runtime", host)
    kernels = (CSRC / "survey.hip").read_text()
    code = re.sub(r"/\*.*?\*/", "", kernels, flags=re.S)
    assert "atomic" not in code.lower() and "sincos" not in code and "__sinf" not in code and "__cosf" not in code


def _wav(path, fs, bps, samples: np.ndarray):
    import struct
    data = samples.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1 if bps != 32 else 3, 2, fs,
                                                                                    fs * 2 * bps // 8, 2 * bps // 8, bps)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(data)) + data)


def test_cli_without_survey_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has neither front end nor survey): it links, --help lists the new
    words, and --offset auto / --decimate auto / --scan exit non-zero saying what the library lacks - not "unrecognized option" -
    and write nothing.  On stdin --offset auto and --scan are refused whatever the library."""
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--offset auto" in h.stderr and "--decimate auto" in h.stderr and "--scan" in h.stderr
    wav = tmp_path / "in.wav"
    _wav(wav, 2400000, 16, np.zeros((16384, 2), dtype=np.int16))
    for extra in (["--offset", "auto"], ["--decimate", "auto"], ["--scan"], ["--offset", "auto", "--decimate", "8"]):
        r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), *extra, str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0
        assert ("no survey" in r.stderr or "no front end" in r.stderr) and "unrecognized" not in r.stderr, r.stderr
        assert r.stdout == "" and not (tmp_path / "out.s").exists() and not list(tmp_path.glob("LRPT_*.s"))
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    for extra in (["--offset", "auto"], ["--scan"]):
        r = subprocess.run([str(cli_exe), "-q", *extra, "--stdout", "-"], capture_output=True, text=True, cwd=tmp_path, stdin=subprocess.DEVNULL)
        assert r.returncode == 1 and "stdin" in r.stderr and r.stdout == "", r.stderr
    r = subprocess.run([str(cli_exe), "-q", "--decimate", "sometimes", str(wav)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "--decimate" in r.stderr


@pytest.mark.timeout(300)
def test_survey_fuzz_under_asan_ubsan(tmp_path):
    exe = tmp_path / "fuzz_survey"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_survey.cpp"), str(CSRC / "survey_detect.cpp"),
                        str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "3000", "7", "2.0"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["cases"] == 3000 and rep["planned"] > 1000 and rep["accepted"] > 500, rep
