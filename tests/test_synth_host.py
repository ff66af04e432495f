"""The host build of the synthetic source (csrc/synth_core.h through meteor_demod_amd.synth) against tests/synth_ref.py: samples
against the signal model within a derived bound, the noise exactly and in its statistics, Es/N0 by an ideal receiver, the
quantisers exactly, and make_stream's fields against their formulas in rational arithmetic."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest

import synth_ref as R
from meteor_demod_amd import synth

FS, RS = 230000.0, 72000.0
RAMPS = ((0.0, 0.0), (40.0, 0.5), (-300.0, -3.0))                      # (Doppler Hz/s, clock ppm/s)
N0S = (0, 1 << 20, (1 << 32) - 1000, 5 * 10 ** 9, 6_074_000_500, 65 * 10 ** 8)


def _unit_stream(seed, oqpsk, ramp, **kw):
    """f32, no noise, no DC, each rail of unit amplitude."""
    st = synth.make_stream(seed, FS, RS, fmt=32, rms=math.sqrt(2.0), dc=(0.0, 0.0), oqpsk=oqpsk,
                           doppler_hz_per_s=ramp[0], clock_ppm_per_s=ramp[1], **kw)
    st.noise_scale = 0.0
    return st


# ---- the reference's own pieces ------------------------------------------------------------------------------------------------

def test_reference_hashes_agree():
    rng = np.random.default_rng(1)
    z = np.concatenate([rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 2000, dtype=np.uint64),
                        np.array([0, 1, R.M64, 1 << 63], dtype=np.uint64)])
    assert [R.mix64(int(v)) for v in z] == [int(v) for v in R.mix64_np(z)]
    j = np.concatenate([np.arange(300, dtype=np.uint64), np.array([R.M64, R.M64 - 1, 1 << 40], dtype=np.uint64)])
    si, sq = R.symbols_np(0xDEADBEEFCAFEF00D, j)
    assert [R.symbol(0xDEADBEEFCAFEF00D, int(v)) for v in j] == list(zip(si.tolist(), sq.tolist()))
    assert abs(np.mean(si.astype(float))) < 0.2 and abs(np.mean(sq.astype(float))) < 0.2


def test_reference_pulse_is_a_unit_energy_nyquist_root():
    t = np.arange(-40 * 64, 40 * 64 + 1) / 64.0
    h = R.rrc(t)
    assert abs(np.sum(h * h) / 64.0 - 1.0) < 1e-3                                 # unit energy
    rc = np.convolve(h, h) / 64.0                                                 # raised cosine: zero at the other symbols
    mid = rc.size // 2
    assert abs(rc[mid] - 1.0) < 1e-3 and np.abs(rc[mid + 64:mid + 64 * 20:64]).max() < 1e-3
    # continuous through both removable singularities
    for t0 in (0.0, 1.0 / (4 * R.ALPHA), -1.0 / (4 * R.ALPHA)):
        assert abs(R.rrc(t0)[0] - R.rrc(t0 + 1e-7)[0]) < 1e-6


def test_vectorised_model_equals_the_scalar_model():
    st = synth.make_stream(5, FS, RS, oqpsk=True, fmt=32, rms=1.0, doppler_hz_per_s=40.0, clock_ppm_per_s=0.5, esn0_db=6.0)
    for n0 in (0, 6_074_000_990):
        z, _ = R.ideal_samples(st, n0, 20)
        for i in range(20):
            a = R.ideal_sample(st, n0 + i)
            assert abs(z[i] - complex(*a)) < 1e-12


# ---- samples against the model -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n0", N0S)
@pytest.mark.parametrize("ramp", RAMPS)
@pytest.mark.parametrize("oqpsk", (False, True))
def test_samples_follow_the_signal_model(oqpsk, ramp, n0):
    """Every sample within the error the construction allows: linear interpolation of the pulse table on both rails, plus the
    carrier word cut to 20 bits.  Before the triangle n(n-1)/2 was kept in 128 bits, the clock-ramp cases from n = 6 074 001 001
    on missed this by 3.6 rail amplitudes."""
    count = 2000
    st = _unit_stream(1000 + n0 % 97, oqpsk, ramp, f0_hz=-1234.5, clock_ppm=17.0)
    got = synth.generate_host(st, count, n0=n0).astype(np.float64)
    want, base = R.ideal_samples(st, n0, count)
    err = np.abs((got[:, 0] + 1j * got[:, 1]) - want)
    bound = math.sqrt(2.0) * R.interpolation_bound() + 2.0 * math.pi * 2.0 ** -20 * np.abs(base)
    print(f"oqpsk={int(oqpsk)} ramp={ramp} n0={n0}: measured {err.max():.3e}, bound {bound.max():.3e} (interpolation "
          f"{math.sqrt(2.0) * R.interpolation_bound():.3e})")
    assert np.all(err <= bound), (err.max(), bound.max(), int(np.argmax(err - bound)))


# ---- noise ---------------------------------------------------------------------------------------------------------------------

def test_noise_is_the_hash_sum_with_its_salts():
    st = synth.make_stream(77, FS, RS, fmt=32, esn0_db=3.0, dc=(0.0, 0.0))
    st.amp = 0.0
    n0 = 123_456_789_012
    got = synth.generate_host(st, 1000, n0=n0)
    want = np.array([[st.noise_scale * R.noise(st.seed, n0 + i, R.SALT_I), st.noise_scale * R.noise(st.seed, n0 + i, R.SALT_Q)]
                     for i in range(1000)]).astype(np.float32)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[:, 0], got[:, 1])


def test_noise_level_and_independence():
    rms, esn0_db = 1.0, 7.0
    st = synth.make_stream(78, FS, RS, fmt=32, esn0_db=esn0_db, rms=rms, dc=(0.0, 0.0))
    st.amp = 0.0
    x = synth.generate_host(st, 1 << 20).astype(np.float64)
    sigma = rms * math.sqrt((FS / RS) / (2.0 * 10.0 ** (esn0_db / 10.0)))
    corr = float(np.corrcoef(x[:, 0], x[:, 1])[0, 1])
    print(f"std {x[:, 0].std():.5f} {x[:, 1].std():.5f} against {sigma:.5f}; corr {corr:+.5f}")
    assert abs(x[:, 0].std() / sigma - 1.0) < 0.005 and abs(x[:, 1].std() / sigma - 1.0) < 0.005
    assert abs(x.mean(axis=0)).max() < 4.0 * sigma / 1024.0                        # zero mean: 4 sigma of the mean of 2^20
    assert abs(corr) < 0.01


# ---- Es/N0 by an ideal receiver ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("oqpsk", (False, True))
@pytest.mark.parametrize("esn0_db", (4.0, 7.0))
def test_esn0_is_what_make_stream_says(esn0_db, oqpsk):
    """Matched filter and symbol-instant decisions on the generator's output: the rail error rate is Q(sqrt(Es/N0)).  Over seeds
    1..6 and 4242 the four cases deviate by +0.4, +0.1, -0.3 and -0.4 sigma on average (single seeds between -2.8 and +2.8): no
    bias either way."""
    nsym, sps = 1 << 16, 4
    st = synth.make_stream(3, 288000.0, 72000.0, f0_hz=0.0, phase0_rad=0.0, sym_phase0=0.0, esn0_db=esn0_db, rms=1.0,
                           dc=(0.0, 0.0), oqpsk=oqpsk, fmt=32)
    assert st.sym_step == 1 << 30
    x = synth.generate_host(st, sps * (nsym + 3 * R.SPAN) + 2).astype(np.float64)
    h = R.rrc(np.arange(-R.SPAN * sps, R.SPAN * sps + 1) / sps)
    j = np.arange(2 * R.SPAN, 2 * R.SPAN + nsym)                                 # the first symbol whose whole pulse is in x
    at = sps * (j - R.SPAN) + R.SPAN * sps                                       # index into the full convolution
    yi = np.convolve(x[:, 0], h)[at]
    yq = np.convolve(x[:, 1], h)[at + (2 if oqpsk else 0)]
    si, sq = R.symbols_np(st.seed, j)
    wrong = int(np.count_nonzero((yi > 0) != (si > 0)) + np.count_nonzero((yq > 0) != (sq > 0)))
    p = 0.5 * math.erfc(math.sqrt(10.0 ** (esn0_db / 10.0) / 2.0))
    n = 2 * nsym
    dev = (wrong - n * p) / math.sqrt(n * p * (1.0 - p))
    print(f"Es/N0 {esn0_db} dB oqpsk={int(oqpsk)}: {wrong} of {n} wrong, expected {n * p:.1f}, {dev:+.2f} sigma")
    assert abs(dev) <= 4.0


# ---- quantisation --------------------------------------------------------------------------------------------------------------

QUANT_VALUES = (0.5, -0.5, 1.5, -1.5, -0.4999, 0.4999, 127.49, 127.5, -128.5, -128.51, 32767.49, 32767.5, -32768.5,
                1e9, -1e9, 1e18, -1e18)


def _dc_only(fmt, vi, vq):
    st = synth.make_stream(9, FS, RS, fmt=fmt, dc=(vi, vq))
    st.amp = 0.0
    st.noise_scale = 0.0
    return st


@pytest.mark.parametrize("fmt", (8, 16, 32))
def test_quantisation_rounds_half_up_and_clips(fmt):
    lo, hi, off = {8: (-128, 127, 128), 16: (-32768, 32767, 0), 32: (None, None, 0)}[fmt]
    for k, v in enumerate(QUANT_VALUES):
        w = QUANT_VALUES[(k + 5) % len(QUANT_VALUES)]
        got = synth.generate_host(_dc_only(fmt, v, w), 3, n0=k * 1000)
        for col, val in ((0, v), (1, w)):
            want = np.float32(val) if fmt == 32 else min(max(math.floor(val + 0.5), lo), hi) + off
            assert np.all(got[:, col] == want), (fmt, val, got[:, col], want)


@pytest.mark.parametrize("fmt,rms,lo,hi,off", ((16, 30000.0, -32768, 32767, 0), (8, 120.0, -128, 127, 128)))
def test_integer_formats_are_the_rounded_float_stream(fmt, rms, lo, hi, off):
    kw = dict(f0_hz=900.0, clock_ppm=-8.0, rms=rms, oqpsk=fmt == 8)
    f = synth.generate_host(synth.make_stream(31, FS, RS, fmt=32, **kw), 20000).astype(np.float64)
    q = synth.generate_host(synth.make_stream(31, FS, RS, fmt=fmt, **kw), 20000).astype(np.float64) - off
    ulp = np.spacing(np.abs(f).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(q - np.clip(f, lo, hi)) <= 0.5 + ulp)
    clipped = float(np.mean((f > hi) | (f < lo)))
    print(f"fmt {fmt}: {100 * clipped:.1f} % of the components clip")
    for col in (0, 1):
        assert q[:, col].min() == lo and q[:, col].max() == hi


# ---- addressability with ramps -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", (1 << 32, 6_074_001_000))
def test_ramped_stream_is_addressable_across(edge):
    st = synth.make_stream(43, FS, RS, f0_hz=-500.0, clock_ppm=4.0, doppler_hz_per_s=40.0, clock_ppm_per_s=0.5, oqpsk=True)
    for k in (1, 1500, 2999):
        a = edge - k
        assert np.array_equal(synth.generate_host(st, 3000, n0=a)[k:], synth.generate_host(st, 3000 - k, n0=a + k))


# ---- make_stream ---------------------------------------------------------------------------------------------------------------

def _near(field: int, exact: Fraction) -> bool:
    """The field is the exact value rounded to an integer, give or take the few float64 roundings of the formula."""
    return abs(field - exact) <= Fraction(1, 2) + abs(exact) * Fraction(1, 2 ** 48)


@pytest.mark.parametrize("f0,ppm,dop,ppm_s", ((1200.0, 0.0, 0.0, 0.0), (-3456.0, 25.0, 40.0, 0.5), (100000.0, -60.0, -300.0, -3.0)))
def test_make_stream_fields(f0, ppm, dop, ppm_s):
    fs, rs, phase0, esn0_db, rms, sp0 = 230000.0, 72000.0, 0.7, 10.0, 6000.0, 0.25
    st = synth.make_stream(12345, fs, rs, f0_hz=f0, phase0_rad=phase0, clock_ppm=ppm, esn0_db=esn0_db, rms=rms, sym_phase0=sp0,
                           doppler_hz_per_s=dop, clock_ppm_per_s=ppm_s)
    F = Fraction
    sym_per_sample = F(rs) * (1 + F(ppm) / 10 ** 6) / F(fs)
    assert _near(st.sym_step, sym_per_sample * 2 ** 32)
    car = F(f0) / F(fs) * 2 ** 32
    assert any(_near(st.car_step, car + w * 2 ** 32) for w in (0, 1)) and 0 <= st.car_step < 2 ** 32
    assert _near(st.car_phase0, F(phase0) / (2 * F(math.pi)) * 2 ** 32)
    assert _near(st.car_ramp48, F(dop) / F(fs) ** 2 * 2 ** 48)
    assert _near(st.clk_ramp64, F(ppm_s) / 10 ** 6 / F(fs) * sym_per_sample * 2 ** 64)
    assert st.sym_phase0 == int(sp0 * 2 ** 32) + (R.SPAN << 32)
    # sigma^2 = rms^2 * sps / (2 Es/N0) per component, over the variance 8 (2^32 - 1) / 12 of the integer sum
    want2 = F(rms) ** 2 / sym_per_sample / (2 * F(10) ** int(esn0_db / 10)) / F(8 * (2 ** 32 - 1), 12)
    assert abs(F(st.noise_scale) ** 2 / want2 - 1) < F(1, 10 ** 12)
    assert F(st.amp) ** 2 * 2 == pytest.approx(rms ** 2, rel=1e-15)
    assert (st.oqpsk, st.fmt, st.seed) == (0, 16, 12345)


def test_make_stream_signs():
    base = synth.make_stream(1, FS, RS, f0_hz=-1000.0)
    assert base.car_step == (1 << 32) - round(1000.0 / FS * 2 ** 32)               # a negative offset wraps modulo one turn
    assert synth.make_stream(1, FS, RS, clock_ppm=50.0).sym_step > base.sym_step   # a fast clock: more symbols per sample
    assert synth.make_stream(1, FS, RS, clock_ppm=-50.0).sym_step < base.sym_step
    up = synth.make_stream(1, FS, RS, doppler_hz_per_s=40.0, clock_ppm_per_s=0.5)
    down = synth.make_stream(1, FS, RS, doppler_hz_per_s=-40.0, clock_ppm_per_s=-0.5)
    assert up.car_ramp48 > 0 > down.car_ramp48 and up.car_ramp48 == -down.car_ramp48      # positive Doppler: car_step grows
    assert up.clk_ramp64 > 0 > down.clk_ramp64 and up.clk_ramp64 == -down.clk_ramp64
