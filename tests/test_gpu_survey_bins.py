"""GPU tests of sv_spectrum / sv_reduce (csrc/survey.hip) bin by bin: one tone on the bin grid per waterfall row, whose exact
Hann periodogram is three bins and nothing else, and a flat spectrum held at every bin.  The helpers are in tests/survey_util.py;
every test prints the figures it asserts on."""
from __future__ import annotations

import numpy as np
import pytest

import survey_util as U

pytestmark = pytest.mark.gpu

FS = 2400000


def _spectrum(x, bps, nfft, rows, gpu_device):
    import torch
    from meteor_demod_amd import DemodConfig, survey
    xd = torch.from_numpy(x).to(f"cuda:{gpu_device}")
    a = survey.spectrum(DemodConfig(samplerate=FS, bps=bps), xd, fft_size=nfft, rows=rows).cpu().numpy()
    assert a.shape == (rows, nfft) and a.dtype == np.float32
    return a.astype(np.float64)


@pytest.mark.parametrize("nfft", [256, 512, 1024, 2048, 4096, 8192, 16384])
def test_one_tone_per_row_on_the_bin_grid(nfft, gpu_device):
    """f32, one launch: row r holds e^{+2 pi i k_r n / N} in three segments of amplitudes 1, 2, 3 (the last row five, 1 .. 5), then
    N / 3 + 1 samples of 1e6 behind the last whole segment.  Exact answer at shifted index (k + N / 2) mod N: mean(a^2) (N / 2)^2,
    a quarter of it on both circular neighbours, 0 elsewhere.  The three bins are within 1e-5 of the peak; every other bin of the
    row is at most 1e-10 of it (a float32 transform on the CPU: 1.2e-7 and 4e-15; the kernel on an MI355X: 4.3e-8 and 4.4e-15 at
    the worst; one wrong point after the first pass: 1.5e-8 at N = 16384).  All N bins up to N = 512, about 60 chosen ones
    beyond.  This pins the output permutation for every digit, the twiddle symmetries, the row of every segment, the idle tail of
    a part, the last row's count and divisor, and that nothing behind the last segment is read."""
    bins = U.tone_bins(nfft)
    rows = len(bins)
    assert rows <= 4096 and (nfft > 512 or rows == nfft)
    x, amps = U.tone_rows(nfft, bins)
    got = _spectrum(x, 32, nfft, rows, gpu_device)
    worst_three = worst_rest = 0.0
    where = None
    for r, (at, peak) in enumerate(U.tone_expected(nfft, bins, amps)):
        three = [(at - 1) % nfft, at, (at + 1) % nfft]
        want = np.array([peak / 4, peak, peak / 4])
        e3 = float(np.abs(got[r, three] - want).max() / peak)
        rest = got[r].copy()
        rest[three] = 0.0
        e0 = float(rest.max() / peak)
        if e0 > worst_rest:
            where = (r, bins[r], int(np.argmax(rest)))
        worst_three, worst_rest = max(worst_three, e3), max(worst_rest, e0)
    print(f"tones nfft={nfft} rows={rows}: the three bins within {worst_three:.3e} of the peak, every other bin at most {worst_rest:.3e} "
          f"of it (row, tone, shifted bin: {where})")
    assert worst_three <= 1e-5, worst_three
    assert worst_rest <= 1e-10, (worst_rest, where)


@pytest.mark.parametrize("bps", [8, 16, 32])
@pytest.mark.parametrize("nfft", [256, 2048, 16384])
def test_flat_spectrum_every_bin(nfft, bps, gpu_device):
    """Seeded white noise (u8 sigma 40 about 128, s16 sigma 3000, f32 sigma 0.3), 64 segments (24 at N = 16384) and an odd tail,
    rows 1 and 5: |got / want - 1| <= 1e-5 against the float64 model at every bin of every row.  A float32 transform on the CPU
    is printed next to it.
    Measured on an MI355X, the largest |got / want - 1| of the kernel / of the float32 CPU transform, over the three formats:
      rows 1:  N = 256: 2.2e-7 / 2.4e-7,  N = 2048: 2.6e-7 / 3.6e-7,  N = 16384: 3.2e-7 / 5.6e-7
      rows 5:  N = 256: 3.5e-7 / 3.6e-7,  N = 2048: 3.7e-7 / 5.9e-7,  N = 16384: 8.8e-7 / 1.1e-6
    (at N = 16384, rows 5, a row is the mean of 4 segments and its smallest bin is 0.016 of the mean)."""
    nseg = 24 if nfft == 16384 else 64
    x = U.noise_input(bps, nseg * nfft + nfft // 3 + 1, seed=bps + nfft)
    for rows in (1, 5):
        want = U.model64(x, bps, nfft, rows)
        yard = U.model32(x, bps, nfft, rows).astype(np.float64)
        got = _spectrum(x, bps, nfft, rows, gpu_device)
        e_k, e_y = float(np.abs(got / want - 1).max()), float(np.abs(yard / want - 1).max())
        print(f"flat bps={bps} nfft={nfft} rows={rows}: max|got/want - 1| kernel {e_k:.3e}, float32 CPU transform {e_y:.3e}, "
              f"smallest bin {want.min() / want.mean():.3f} of the mean")
        assert e_k <= 1e-5, (rows, e_k, e_y)
