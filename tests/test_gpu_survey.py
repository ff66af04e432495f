"""GPU tests of the survey (include/meteor_demod_amd_survey.h): the spectrum kernel against a float64 model, its determinism,
and the capability it adds: finding LRPT in a wide recording next to stronger signals that are not LRPT, confirming it, and
handing the front end an offset on which the demodulator locks.  Every test prints the figures it asserts on."""
from __future__ import annotations

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 2400000
RMS = 2000.0          # per signal: the s16 sum of every scene below clips on fewer than 1e-4 of its samples (asserted in _scene)
_NP = {8: np.uint8, 16: np.int16, 32: np.float32}


# ---------------------------------------------------------------------------------------------------------------- spectrum
def _tone_input(bps, n, seed):
    """Noise plus one full-scale tone off the bin grid: the largest bin and the floor are 60+ dB apart."""
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * 0.1234567 * np.arange(n) + 0.3
    if bps == 8:
        v = 128.0 + 127.0 * np.stack([np.cos(ph), np.sin(ph)], axis=1) + rng.normal(0, 0.5, size=(n, 2))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if bps == 16:
        v = 30000.0 * np.stack([np.cos(ph), np.sin(ph)], axis=1) + rng.normal(0, 20.0, size=(n, 2))
        return np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    return (np.stack([np.cos(ph), np.sin(ph)], axis=1) + rng.normal(0, 1e-3, size=(n, 2))).astype(np.float32)


def _model(x, bps, nfft, rows):
    """float64: the same segments, the window as the kernel defines it (periodic Hann), np.fft, the mean of |X|^2 per row.
    Returns (psd [rows, nfft], segment count per row)."""
    xc = x.astype(np.float64) - (128.0 if bps == 8 else 0.0)
    z = xc[:, 0] + 1j * xc[:, 1]
    nseg = len(z) // nfft
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)
    per = nseg // rows
    out, counts = [], []
    for r in range(rows):
        lo, hi = r * per, (nseg if r == rows - 1 else (r + 1) * per)
        seg = z[lo * nfft: hi * nfft].reshape(hi - lo, nfft) * w
        out.append((np.abs(np.fft.fftshift(np.fft.fft(seg, axis=1), axes=1)) ** 2).mean(axis=0))
        counts.append(hi - lo)
    return np.array(out), np.array(counts)


@pytest.mark.parametrize("bps", [8, 16, 32])
@pytest.mark.parametrize("nfft", [256, 1024, 4096, 16384])
def test_spectrum_matches_float64_model(bps, nfft, gpu_device):
    """u8 / s16 / f32 x fft_size {256, 1024, 4096, 16384} x rows {1, 7}, lengths that are a multiple of nothing: max |error| over
    a row <= 1e-4 of that row's largest bin.  Two runs give the same bytes; the rows of the waterfall, weighted by their segment
    counts, give the plain spectrum to the same bar."""
    import torch
    from meteor_demod_amd import DemodConfig, survey
    nseg = max(23, 200000 // nfft)
    n = nseg * nfft + nfft // 3 + 1
    x = _tone_input(bps, n, seed=bps + nfft)
    xd = torch.from_numpy(x).to(f"cuda:{gpu_device}")
    cfg = DemodConfig(samplerate=FS, bps=bps)
    got = {}
    for rows in (1, 7):
        want, counts = _model(x, bps, nfft, rows)
        a = survey.spectrum(cfg, xd, fft_size=nfft, rows=rows).cpu().numpy()
        b = survey.spectrum(cfg, xd, fft_size=nfft, rows=rows).cpu().numpy()
        assert a.shape == (rows, nfft) and a.dtype == np.float32
        assert a.tobytes() == b.tobytes(), "two runs differ"
        for r in range(rows):
            peak, floor = want[r].max(), np.median(want[r])
            assert peak / floor >= 1e6, (peak / floor)              # the input does what it is meant to
            ratio = np.abs(a[r].astype(np.float64) - want[r]).max() / peak
            print(f"spectrum bps={bps} nfft={nfft} rows={rows} row={r}: max|err|/peak = {ratio:.3e}")
            assert ratio <= 1e-4, (bps, nfft, rows, r, ratio)
            assert int(np.argmax(a[r])) == int(np.argmax(want[r]))
        got[rows] = (a.astype(np.float64), counts)
    a7, c7 = got[7]
    merged = (a7 * c7[:, None]).sum(axis=0) / c7.sum()
    one = got[1][0][0]
    ratio = np.abs(merged - one).max() / one.max()
    print(f"spectrum bps={bps} nfft={nfft}: rows=7 merged against rows=1: {ratio:.3e}")
    assert ratio <= 1e-4


def test_spectrum_default_size_and_odd_log2(gpu_device):
    """fft_size 512, 2048 and 8192 (a last radix-2 pass) against the model, and the default size from the plan."""
    import torch
    from meteor_demod_amd import DemodConfig, survey
    x = _tone_input(16, 8192 * 9 + 77, seed=3)
    xd = torch.from_numpy(x).to(f"cuda:{gpu_device}")
    for nfft in (512, 2048, 8192):
        want, _ = _model(x, 16, nfft, 2)
        a = survey.spectrum(DemodConfig(samplerate=FS, bps=16), xd, fft_size=nfft, rows=2).cpu().numpy()
        ratio = max(np.abs(a[r] - want[r]).max() / want[r].max() for r in range(2))
        print(f"spectrum nfft={nfft}: {ratio:.3e}")
        assert ratio <= 1e-4
    assert survey.spectrum(DemodConfig(samplerate=FS, bps=16), xd).shape == (1, 4096)
    assert survey.spectrum(DemodConfig(samplerate=230000, bps=16), xd).shape == (1, 512)


def test_spectrum_refusals(gpu_device):
    import torch
    from meteor_demod_amd import DemodConfig, _capi, survey
    xd = torch.zeros((5000, 2), dtype=torch.int16, device=f"cuda:{gpu_device}")
    cfg = DemodConfig(samplerate=FS, bps=16)
    for kw, word in ((dict(fft_size=1000), "fft_size"), (dict(fft_size=128), "fft_size"), (dict(fft_size=32768), "fft_size"),
                     (dict(fft_size=256, rows=0), "n_rows"), (dict(fft_size=1024, rows=5), "n_rows"), (dict(fft_size=8192), "segments")):
        with pytest.raises(_capi.MdemodError) as e:
            survey.spectrum(cfg, xd, **kw)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail


# ------------------------------------------------------------------------------------------------------------------ scenes
def _noise(n, sigma, seed, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn((n, 2), generator=g, device=dev, dtype=torch.float32) * sigma


def _sigma(esn0_db, symrate=72000, rms=RMS):
    """The per-component noise of a synth stream of that Es/N0 (synth.make_stream)."""
    return rms * math.sqrt(FS / symrate / (2.0 * 10.0 ** (esn0_db / 10.0)))


def _scene(n, gpu_device, lrpt=(), fm=False, carrier=False, noise_sigma=0.0, seed=1, blank_first_half=False):
    """A 2.4 MS/s s16 recording on the device.  lrpt: (offset_hz, esn0_db, seed, symrate, oqpsk) each; the FIRST carries the
    noise of its Es/N0, the others are near-noiseless (60 dB) so that the floor is the first one's.  fm: an FM-modulated tone
    (+-17 kHz deviation at 2.4 kHz) of RMS `RMS` at -600 kHz; carrier: a carrier of twice that RMS at +700 kHz; noise_sigma:
    white noise per component on top.  Returns (iq int16 [n, 2], [streams])."""
    import torch
    from meteor_demod_amd import synth
    dev = f"cuda:{gpu_device}"
    acc = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    streams = []
    for i, (off, esn0, sd, symrate, oqpsk) in enumerate(lrpt):
        st = synth.make_stream(sd, FS, symrate, f0_hz=off, esn0_db=esn0 if i == 0 else 60.0, rms=RMS, dc=(0.0, 0.0), oqpsk=oqpsk)
        streams.append(st)
        acc += synth.generate_device([st], n, device=gpu_device)[0].to(torch.float32)
    if blank_first_half:
        acc[: n // 2] = _noise(n // 2, _sigma(lrpt[0][1], lrpt[0][3]), seed + 7, dev)
    t = torch.arange(n, dtype=torch.float64, device=dev)
    if fm:
        ph = 2 * math.pi * (-600000.0 / FS) * t + (17000.0 / 2400.0) * torch.sin(2 * math.pi * (2400.0 / FS) * t)
        acc += (RMS * torch.stack([torch.cos(ph), torch.sin(ph)], dim=1)).to(torch.float32)
    if carrier:
        ph = 2 * math.pi * (700000.0 / FS) * t
        acc += (2 * RMS * torch.stack([torch.cos(ph), torch.sin(ph)], dim=1)).to(torch.float32)
    del t
    if noise_sigma:
        acc += _noise(n, noise_sigma, seed, dev)
    clipped = float(((acc > 32767.0) | (acc < -32768.0)).float().mean())
    assert clipped < 1e-4, clipped
    return acc.round().clamp(-32768, 32767).to(torch.int16).contiguous(), streams


def _show(tag, hits):
    for h in hits:
        print(f"{tag}: offset {h.offset_hz:+.1f} Hz (coarse {h.coarse_offset_hz:+.1f}) psd_snr {h.psd_snr_db:.2f} dB clock_q {h.clock_quality:.2f} "
              f"carrier_q {h.carrier_quality:.2f} row {h.best_row} confirmed {h.confirmed} refined {h.refined}")
    if not hits:
        print(f"{tag}: no hit")


def _near(hits, f, tol):
    return [h for h in hits if abs(h.coarse_offset_hz - f) <= tol]


# -------------------------------------------------------------------------------------------------------------- capability
@pytest.mark.parametrize("esn0_db,symrate,oqpsk", [(15.0, 72000, False), (6.0, 72000, False), (15.0, 80000, True)])
def test_survey_finds_lrpt_next_to_stronger_signals(esn0_db, symrate, oqpsk, gpu_device):
    """2^24 samples: LRPT at +301 200 Hz, an FM tone of equal RMS at -600 kHz, a carrier of twice the RMS at +700 kHz.  The LRPT
    hit comes first and confirmed, within 100 Hz; the two others are hits and NOT confirmed.  FrontEnd(hit.offset_hz, 8) on the
    same samples then locks within the first quarter.  At Es/N0 = 15 dB the demodulated symbols pass the bars of
    test_gpu_frontend.py::test_off_centre_signal_next_to_an_interferer (rail error rate < 1e-4, no pairing change, no unresolved
    block).  At 6 dB no demodulator can reach that error rate: uncoded QPSK at Es/N0 = 6 dB errs on Q(sqrt(Es/N0)) = 2.3e-2 of the
    rails, so there the rate is held to 3.8e-2 (the same with 1 dB of implementation loss; measured 2.41e-2) and every other bar
    stays (lock within the first quarter, no pairing change, no unresolved block)."""
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig, survey, synth
    n = 1 << 24
    x, (sig,) = _scene(n, gpu_device, lrpt=[(301200.0, esn0_db, 5, symrate, oqpsk)], fm=True, carrier=True)
    cfg = DemodConfig(samplerate=FS, symrate=symrate, oqpsk=oqpsk)
    hits = survey.survey(cfg, x)
    _show(f"lrpt {symrate} esn0 {esn0_db}", hits)
    assert hits and hits[0].confirmed
    assert abs(hits[0].offset_hz - 301200.0) <= 100.0, hits[0]
    assert abs(hits[0].coarse_offset_hz - 301200.0) <= FS / 4096
    for f in (-600000.0, 700000.0):
        other = _near(hits, f, 0.8 * symrate)
        assert other and not any(h.confirmed for h in other), (f, other)
    assert sum(h.confirmed for h in hits) == 1
    with FrontEnd(cfg, FrontEndConfig(hits[0].offset_hz, 8), 1) as f:
        soft = f.process(x.reshape(1, n, 2))
        torch.cuda.synchronize()
        st = f.status()[0]
        assert st.locked_once and 0 <= st.first_lock_symbol < st.symbols_this_call // 4
        out = soft[0, : st.symbols_this_call].contiguous()
        tc = synth.truth_check(sig, out, first_symbol=int(st.first_lock_symbol) + 20000)
    print(f"lrpt {symrate} esn0 {esn0_db}: lock at {st.first_lock_symbol}, {tc}")
    assert tc["symbols_compared"] > 250000, tc
    assert tc["pairing_changes"] == 0 and tc["unresolved_blocks"] == 0, tc
    assert tc["rail_error_rate"] < (1e-4 if esn0_db >= 15.0 else 3.8e-2), tc


def test_survey_negatives_noise_alone(gpu_device):
    """White noise: nothing is confirmed (and at the default min_snr_db nothing is even a candidate)."""
    from meteor_demod_amd import DemodConfig, survey
    x, _ = _scene(1 << 24, gpu_device, noise_sigma=4000.0)
    hits = survey.survey(DemodConfig(samplerate=FS), x)
    _show("noise alone", hits)
    assert not any(h.confirmed for h in hits)
    assert not hits
    loose = survey.survey(DemodConfig(samplerate=FS), x, min_snr_db=-40.0)
    _show("noise alone, min_snr_db -40", loose)
    assert loose and not any(h.confirmed for h in loose)


def test_survey_negatives_fm_and_carrier_without_lrpt(gpu_device):
    from meteor_demod_amd import DemodConfig, survey
    x, _ = _scene(1 << 24, gpu_device, fm=True, carrier=True, noise_sigma=_sigma(15.0))
    hits = survey.survey(DemodConfig(samplerate=FS), x)
    _show("fm + carrier", hits)
    assert _near(hits, -600000.0, 57600.0) and _near(hits, 700000.0, 57600.0)
    assert not any(h.confirmed for h in hits)


def test_survey_negatives_other_symbol_rate(gpu_device):
    """An 80 k OQPSK signal surveyed as 72 k QPSK: found by the spectrum, not confirmed by the clock line."""
    from meteor_demod_amd import DemodConfig, survey
    x, _ = _scene(1 << 24, gpu_device, lrpt=[(301200.0, 15.0, 5, 80000, True)])
    hits = survey.survey(DemodConfig(samplerate=FS, symrate=72000), x)
    _show("80k oqpsk as 72k", hits)
    assert _near(hits, 301200.0, 57600.0)
    assert not any(h.confirmed for h in hits)


def test_survey_two_signals_in_one_file(gpu_device):
    from meteor_demod_amd import DemodConfig, survey
    x, _ = _scene(1 << 24, gpu_device, lrpt=[(-400000.0, 15.0, 5, 72000, False), (400000.0, 15.0, 77, 72000, False)])
    hits = survey.survey(DemodConfig(samplerate=FS), x)
    _show("two signals", hits)
    good = [h for h in hits if h.confirmed]
    assert len(good) == 2
    assert sorted(round(h.offset_hz / 1000) for h in good) == [-400, 400]
    for h in good:
        assert min(abs(h.offset_hz - 400000.0), abs(h.offset_hz + 400000.0)) <= 100.0, h


def test_survey_waterfall_signal_in_the_second_half(gpu_device):
    """The first half of the recording is noise: best_row lies in the second half (rows = 8) and the hit is still confirmed,
    because the confirmation window is taken where the signal is."""
    from meteor_demod_amd import DemodConfig, survey
    x, _ = _scene(1 << 24, gpu_device, lrpt=[(301200.0, 15.0, 5, 72000, False)], blank_first_half=True)
    hits = survey.survey(DemodConfig(samplerate=FS), x, n_rows=8)
    _show("second half", hits)
    assert hits and hits[0].confirmed and hits[0].best_row >= 4
    assert abs(hits[0].offset_hz - 301200.0) <= 100.0


def test_survey_host_equals_device(gpu_device):
    """mdemod_survey_host on the same samples in host memory (one piece): the same hits."""
    from meteor_demod_amd import DemodConfig, survey
    x, _ = _scene(1 << 22, gpu_device, lrpt=[(301200.0, 15.0, 5, 72000, False)], carrier=True)
    cfg = DemodConfig(samplerate=FS)
    a, b = survey.survey(cfg, x), survey.survey(cfg, x.cpu().numpy())
    _show("device", a)
    _show("host", b)
    assert a == b and a and a[0].confirmed


# --------------------------------------------------------------------------------------------------------------------- CLI
def _wav(path, fs, bps, data: bytes):
    import struct
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1 if bps != 32 else 3, 2, fs,
                                                                                    fs * 2 * bps // 8, 2 * bps // 8, bps)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(data)) + data)


def test_cli_offset_auto_and_scan(tmp_path, gpu_device):
    """--scan prints one confirmed line within 100 Hz; --offset auto writes the bytes of --offset <that offset> --decimate <auto's
    D>, exact and --tiled; the noise-only WAV exits 1, is named, and leaves no output file; stdin is refused; a batch of two files
    with different offsets gets each its own."""
    import subprocess
    from conftest import ROOT
    from meteor_demod_amd import DemodConfig, survey_plan
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    n = 1 << 22
    x, _ = _scene(n, gpu_device, lrpt=[(301200.0, 15.0, 5, 72000, False)], fm=True, carrier=True)
    y, _ = _scene(n, gpu_device, lrpt=[(-412345.0, 15.0, 9, 72000, False)], carrier=True)
    z, _ = _scene(n, gpu_device, noise_sigma=4000.0)
    wavs = {}
    for name, t in (("sig", x), ("other", y), ("noise", z)):
        wavs[name] = tmp_path / f"{name}.wav"
        _wav(wavs[name], FS, 16, t.cpu().numpy().tobytes())
    d = survey_plan(DemodConfig(samplerate=FS))[1]

    def cli(*args, stdin=None):
        return subprocess.run([str(cli_exe), "-q", "-B", *map(str, args)], capture_output=True, text=True, cwd=tmp_path, timeout=600, stdin=stdin)

    p = cli("--scan", wavs["sig"])
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    lines = [ln.split() for ln in p.stdout.strip().splitlines()]
    assert all(len(ln) == 5 for ln in lines) and len(lines) >= 3
    good = [ln for ln in lines if ln[4] == "1"]
    assert len(good) == 1 and lines[0] == good[0] and abs(float(good[0][0]) - 301200.0) <= 100.0
    assert not list(tmp_path.glob("*.s"))
    for mode in ([], ["--tiled"]):
        a, b = tmp_path / "a.s", tmp_path / "b.s"
        p = cli(*mode, "--offset", "auto", "-o", a, wavs["sig"])
        assert p.returncode == 0, p.stderr
        p = cli(*mode, "--offset", good[0][0], "--decimate", d, "-o", b, wavs["sig"])
        assert p.returncode == 0, p.stderr
        assert a.stat().st_size > 100000 and a.read_bytes() == b.read_bytes(), mode
    out = tmp_path / "none.s"
    p = cli("--offset", "auto", "-o", out, wavs["noise"])
    assert p.returncode == 1 and "noise.wav" in p.stderr, (p.returncode, p.stderr)
    assert not out.exists()
    p = cli("--scan", wavs["noise"])
    assert p.returncode == 0 and p.stdout.strip() == "", (p.stdout, p.stderr)
    with open(wavs["sig"], "rb") as f:
        p = cli("--offset", "auto", "--stdout", "-", stdin=f)
    assert p.returncode == 1 and "stdin" in p.stderr and p.stdout == ""
    # a batch: each file its own offset = each file alone
    p = cli("--offset", "auto", wavs["sig"], wavs["other"])
    assert p.returncode == 0, p.stderr
    for name in ("sig", "other"):
        one = tmp_path / f"{name}_alone.s"
        p = cli("--offset", "auto", "-o", one, wavs[name])
        assert p.returncode == 0, p.stderr
        batch = tmp_path / f"{name}.wav.s"
        assert batch.stat().st_size > 100000 and batch.read_bytes() == one.read_bytes(), name
    p = cli("--scan", wavs["other"])
    other = [ln.split() for ln in p.stdout.strip().splitlines() if ln.split()[4] == "1"]
    assert len(other) == 1 and abs(float(other[0][0]) + 412345.0) <= 100.0
