"""Helpers of the per-bin spectrum tests (no GPU): tones on the bin grid, one bin per waterfall row, with their exact Hann
periodogram; white noise in the three input formats; the float64 model and a float32 CPU transform as a yardstick.

Why tones on the grid: e^{+2 pi i k n / N} under the periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / N) transforms to N / 2
at bin k, -N / 4 at k - 1 and k + 1 (circular) and nothing anywhere else.  Every other bin of the row is then rounding alone, so
a misplaced output, a wrong twiddle or a segment in the wrong row shows as a bin that should be empty."""
from __future__ import annotations

import numpy as np

_NP = {8: np.uint8, 16: np.int16, 32: np.float32}
TAIL_VALUE = 1e6


def tone_bins(nfft: int, seed: int = 0) -> list:
    """All bins up to 512 points; beyond, the edges of the octants and of the spectrum, every power of two and three times every
    power of two below nfft, and 32 seeded bins."""
    if nfft <= 512:
        return list(range(nfft))
    ks = {0, 1, nfft // 8 - 1, nfft // 8, nfft // 8 + 1, nfft // 4, nfft // 2 - 1, nfft // 2, nfft // 2 + 1, nfft - 1}
    p = 1
    while p < nfft:
        ks.add(p)
        if 3 * p < nfft:
            ks.add(3 * p)
        p *= 2
    rng = np.random.default_rng(nfft + seed)
    ks.update(int(v) for v in rng.integers(0, nfft, size=32))
    return sorted(ks)


def tone_rows(nfft: int, bins) -> tuple:
    """(x float32 [n, 2], amplitudes per row).  Row r: three segments of e^{+2 pi i k_r n / N} with amplitudes 1, 2, 3; the last row
    five, amplitudes 1 .. 5, since n // nfft = 3 rows + 2; then nfft / 3 + 1 samples of 1e6 that no segment holds."""
    rows = len(bins)
    n = np.arange(nfft, dtype=np.int64)
    amps = [[1.0, 2.0, 3.0]] * (rows - 1) + [[1.0, 2.0, 3.0, 4.0, 5.0]]
    segs = []
    for k, aa in zip(bins, amps):
        ph = 2 * np.pi * ((k * n) % nfft).astype(np.float64) / nfft
        tone = np.stack([np.cos(ph), np.sin(ph)], axis=1)
        segs += [a * tone for a in aa]
    tail = np.full((nfft // 3 + 1, 2), TAIL_VALUE)
    x = np.concatenate(segs + [tail]).astype(np.float32)
    assert len(x) // nfft == 3 * rows + 2
    return x, amps


def tone_expected(nfft: int, bins, amps):
    """Per row: (shifted index of the peak, peak value mean(a^2) (N / 2)^2); both circular neighbours hold a quarter of it."""
    return [((k + nfft // 2) % nfft, float(np.mean(np.square(a))) * (nfft / 2.0) ** 2) for k, a in zip(bins, amps)]


def noise_input(bps: int, n: int, seed: int) -> np.ndarray:
    """White noise: u8 sigma 40 about 128, s16 sigma 3000, f32 sigma 0.3."""
    rng = np.random.default_rng(seed)
    if bps == 8:
        return np.clip(np.rint(128.0 + rng.normal(0, 40.0, size=(n, 2))), 0, 255).astype(np.uint8)
    if bps == 16:
        return np.clip(np.rint(rng.normal(0, 3000.0, size=(n, 2))), -32768, 32767).astype(np.int16)
    return rng.normal(0, 0.3, size=(n, 2)).astype(np.float32)


def _rows(x, bps, nfft, rows, dtype):
    xc = x.astype(dtype) - dtype(128 if bps == 8 else 0)
    z = xc[:, 0] + 1j * xc[:, 1]
    nseg = len(z) // nfft
    per = nseg // rows
    for r in range(rows):
        lo, hi = r * per, (nseg if r == rows - 1 else (r + 1) * per)
        yield z[lo * nfft: hi * nfft].reshape(hi - lo, nfft)


def model64(x, bps, nfft, rows) -> np.ndarray:
    """float64: row r is segments r per .. (r + 1) per - 1 (the last row: all the rest), periodic Hann, np.fft, the mean of |X|^2,
    bin 0 = -fs / 2.  [rows, nfft]."""
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)
    return np.array([(np.abs(np.fft.fftshift(np.fft.fft(seg * w, axis=1), axes=1)) ** 2).mean(axis=0)
                     for seg in _rows(x, bps, nfft, rows, np.float64)])


def model32(x, bps, nfft, rows) -> np.ndarray:
    """The same in float32 on the CPU (torch, complex64 transform, float32 sums): what single precision gives without this
    library's kernel."""
    import torch
    w = torch.from_numpy((0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)).astype(np.float32))
    out = []
    for seg in _rows(x, bps, nfft, rows, np.float32):
        t = torch.from_numpy(seg.astype(np.complex64)) * w
        p = torch.fft.fftshift(torch.fft.fft(t, dim=1), dim=1)
        out.append((p.real * p.real + p.imag * p.imag).mean(dim=0).numpy())
    return np.array(out)
