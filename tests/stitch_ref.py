"""Plain models of the recording stitcher's kernels (csrc/recording.hip), restated from the comments there and NOTEBOOK.md 3.1.

numpy with Python integers / int64 (seam matches, assembly) and float64 (power, carrier and clock estimators).  Nothing here
imports the library: tests/test_gpu_stitch_kernels.py holds the kernels to these functions, tests/test_stitch_ref_host.py
holds these functions to planted answers.

Exactness of the seam matches.  A sum over K symbols of products of two int8 values is at most K * 2 * 128^2 in magnitude; for
K <= 1024 that is 2^25, so 4 * best^2 <= 2^52 and Ea * Eb <= 2^50: both sides of the weak rule are integers below 2^53, the
kernels' double arithmetic holds them exactly, and the models use Python integers.
"""
from __future__ import annotations

import math

import numpy as np

K_EXACT_MAX = 1024


def rot_sym(i, q, k):
    """(i + jq) * j^k on integers (no wrap)."""
    k &= 3
    if k == 0:
        return i, q
    if k == 1:
        return -q, i
    if k == 2:
        return -i, -q
    return q, -i


def _as_pairs(x):
    x = np.asarray(x).astype(np.int64)
    return x.reshape(-1, 2)


def _tail(x, n):
    """The last n symbols of x, zeros in front of a short one."""
    x = _as_pairs(x)
    out = np.zeros((n, 2), dtype=np.int64)
    m = min(n, len(x))
    if m:
        out[n - m:] = x[len(x) - m:]
    return out


def _head(x, n):
    """The first n symbols of x, zeros behind a short one."""
    x = _as_pairs(x)
    out = np.zeros((n, 2), dtype=np.int64)
    m = min(n, len(x))
    out[:m] = x[:m]
    return out


def _corr(a, b):
    """sum a * conj(b) as two Python integers."""
    re = int((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).sum())
    im = int((a[:, 1] * b[:, 0] - a[:, 0] * b[:, 1]).sum())
    return re, im


def _energy(a):
    return int((a * a).sum())


def _pick_shift_rot(cands):
    """cands: [(shift, re, im)] in the kernels' order.  score(r) = Re(c * j^-r): re, im, -re, -im.  Within a shift the first
    maximum over r = 0, 1, 2, 3; over the shifts the first maximum in the order given."""
    best = None
    for shift, re, im in cands:
        sc = [re, im, -re, -im]
        r = 0
        for k in range(1, 4):
            if sc[k] > sc[r]:
                r = k
        if best is None or sc[r] > best[0]:
            best = (sc[r], shift, r)
    return best


def _weak(best, ea, eb, force_weak):
    """Less than half of a perfect match with the amplitudes taken out, or nothing positive at all, or told so."""
    return best <= 0 or 4 * best * best < ea * eb or bool(force_weak)


def _result(best, shift, rot, ea, eb, force_weak, **extra):
    weak = _weak(best, ea, eb, force_weak)
    d = dict(shift=0 if weak else shift, rot=0 if weak else rot, weak=int(weak), best=best, ea=ea, eb=eb, raw_shift=shift, raw_rot=rot)
    d.update(extra)
    return d


def match_tails(a, b, K, b_rot=0, force_weak=0):
    """match_kernel: tails of K + 1 symbols aligned at their ends, B turned by b_rot quarter turns first.
    shift 0: a[1..K] vs b[1..K]; +1: a[0..K-1] vs b[1..K]; -1: a[1..K] vs b[0..K-1]; tried in that order."""
    assert 1 <= K <= K_EXACT_MAX
    A, B = _tail(a, K + 1), _tail(b, K + 1)
    bi, bq = rot_sym(B[:, 0], B[:, 1], b_rot)
    B = np.stack((bi, bq), axis=1)
    cands = [(0, *_corr(A[1:], B[1:])), (1, *_corr(A[:K], B[1:])), (-1, *_corr(A[1:], B[:K]))]
    best, shift, rot = _pick_shift_rot(cands)
    return _result(best, shift, rot, _energy(A[1:]), _energy(B[1:]), force_weak, scores=cands)


def match_heads(a, b, K, force_weak=0):
    """match_heads_kernel: both start on the same sample (index 0), symbols past cnt are zeros.
    shift 0: a[0..K-1] vs b[0..K-1]; +1: a[1..K] vs b[0..K-1]; -1: a[0..K-1] vs b[1..K]."""
    assert 1 <= K <= K_EXACT_MAX
    A, B = _head(a, K + 1), _head(b, K + 1)
    cands = [(0, *_corr(A[:K], B[:K])), (1, *_corr(A[1:], B[:K])), (-1, *_corr(A[:K], B[1:]))]
    best, shift, rot = _pick_shift_rot(cands)
    return _result(best, shift, rot, _energy(A[:K]), _energy(B[:K]), force_weak, scores=cands)


def match_rails(a, b, K, force_weak=0):
    """match_rails_kernel (OQPSK): tails of K + 2 symbols aligned at their ends, a = A[1..K]; for every quarter turn r the I rail
    and the Q rail of B * j^r are each correlated with a's at shifts -1, 0, +1 and take their best; the first r (0 first, then
    strictly greater) with the largest sum of the two wins.  No shift is reported.  `pairing`: per r the shifts the two rails
    took (first maximum in the order -1, 0, +1) - what the tests classify their cases with."""
    assert 1 <= K <= K_EXACT_MAX
    A, B = _tail(a, K + 2), _tail(b, K + 2)
    a1 = A[1:K + 1]
    best, br, pairing, tots = None, 0, [], []
    for r in range(4):
        mi, mq = rot_sym(B[:, 0], B[:, 1], r)
        si = [int((a1[:, 0] * mi[d:d + K]).sum()) for d in range(3)]
        sq = [int((a1[:, 1] * mq[d:d + K]).sum()) for d in range(3)]
        pairing.append((si.index(max(si)) - 1, sq.index(max(sq)) - 1))
        tot = max(si) + max(sq)
        tots.append(tot)
        if best is None or tot > best:
            best, br = tot, r
    return _result(best, 0, br, _energy(a1), _energy(B[1:K + 1]), force_weak, pairing=pairing, tots=tots)


def wrap8(x):
    """An integer as the int8 that holds its low byte: -(-128) = 128 stays -128."""
    return ((np.asarray(x, dtype=np.int64) + 128) & 0xFF) - 128


def assemble(out, src, src_off, keep, rot, head_off, head_rot, dst):
    """assemble_kernel: for every tile, the optional head symbol src[head_off] turned by head_rot, then keep symbols from
    src[src_off] turned by rot, written from symbol dst of `out` (int8 [n, 2], changed in place and returned).  Negation wraps
    as int8 on every path."""
    src = _as_pairs(src)
    for t in range(len(keep)):
        at = int(dst[t])
        if head_off[t] >= 0:
            i, q = rot_sym(src[int(head_off[t]), 0], src[int(head_off[t]), 1], int(head_rot[t]))
            out[at, 0], out[at, 1] = wrap8(i), wrap8(q)
            at += 1
        seg = src[int(src_off[t]): int(src_off[t]) + int(keep[t])]
        i, q = rot_sym(seg[:, 0], seg[:, 1], int(rot[t]))
        out[at: at + int(keep[t]), 0] = wrap8(i)
        out[at: at + int(keep[t]), 1] = wrap8(q)
    return out


def to_float(iq):
    """Samples [n, 2] of any of the three formats as float64 pairs; u8 is value - 128."""
    iq = np.asarray(iq)
    x = iq.astype(np.float64)
    if iq.dtype == np.uint8:
        x = x - 128.0
    return x


def window_power(iq, start, n):
    """Mean |z - mean|^2 of n samples from `start`; 0 for an empty window."""
    if n == 0:
        return 0.0
    x = to_float(iq[start:start + n])
    z = x[:, 0] + 1j * x[:, 1]
    return float(np.mean(np.abs(z - z.mean()) ** 2))


# ---- estimators --------------------------------------------------------------------------------------------------------------

def carrier_geometry(samplerate, symrate, window_samples):
    """carrier_window() and the entry's `pre`: (nwin, decim, log2_nf, kmax, pre)."""
    fs, sr = float(samplerate), float(symrate)
    n = 4096
    while n * 2 <= min(int(window_samples), 1 << 18):
        n *= 2
    band_hz = 4 * 0.33 * sr / (2 * math.pi)
    d = 1
    while d < 16 and fs / (2.0 * (d * 2)) >= 1.25 * band_hz:
        d *= 2
    while n // d > 16384:
        n //= 2
    while d > 1 and n // d < 4096:
        d //= 2
    l2 = (n // d).bit_length() - 1
    kmax = min(n // d // 2 - 2, int(band_hz / fs * n) + 2)
    pre = 1
    while pre * 2 <= d and pre * 2 * 3.0 <= fs / sr:
        pre *= 2
    return n, d, l2, kmax, pre


def clock_geometry(samplerate, symrate, oqpsk, window_samples):
    """The clock entry's (nwin, decim, log2_nf, kmax, knoise)."""
    n = 4096
    while n * 2 <= min(int(window_samples), 1 << 18):
        n *= 2
    f_nom = float(symrate) / float(samplerate)
    kmax = min(2048 - 2, int(f_nom / 4096.0 * n) + (12 if oqpsk else 3))
    knoise = min(2048 - 2, max(128, 2 * kmax))
    return n, n >> 12, 12, kmax, knoise


def _window_samples(x, start, nwin):
    """nwin samples from `start` as complex128; samples past the end repeat the last one."""
    idx = np.minimum(int(start) + np.arange(nwin, dtype=np.int64), len(x) - 1)
    return x[idx, 0] + 1j * x[idx, 1]


def _hann(nf):
    return 0.5 - 0.5 * np.cos(np.pi * (2.0 / (nf - 1)) * np.arange(nf))


def grandke(a, b, c):
    """Offset of a Hann-windowed line from the largest magnitude b and its neighbours a (below) and c (above)."""
    if not b > 0.0:
        return 0.0
    al = (c if c >= a else a) / b
    delta = min(max((2.0 * al - 1.0) / (al + 1.0), 0.0), 0.5)
    return -delta if c < a else delta


def _peak(spec, kmax, kband, round_mags):
    """Largest |X|^2 among bins strictly inside +-kmax (lowest index on ties), Grandke offset, quality = peak magnitude over
    the mean magnitude of the 2 * kband + 1 bins around 0.  Also the ratio of the largest to the second largest in-band
    magnitude that is not its neighbour (the margin the tests ask of their inputs)."""
    nf = len(spec)
    ks = np.arange(-kband, kband + 1)
    p = np.abs(spec[ks % nf]) ** 2
    inside = (ks > -kmax) & (ks < kmax)
    k = int(ks[inside][np.argmax(p[inside])])
    a, b, c = (math.sqrt(float(np.abs(spec[(k + o) % nf]) ** 2)) for o in (-1, 0, 1))
    if round_mags:
        a, b, c = float(np.float32(a)), float(np.float32(b)), float(np.float32(c))
    delta = grandke(a, b, c)
    quality = b / (float(np.sqrt(p).sum()) / (2 * kband + 1) + 1e-30)
    far = inside & (np.abs(ks - k) > 1)
    second = math.sqrt(float(p[far].max())) if far.any() else 0.0
    margin = b / second if second > 0 else math.inf
    return k, delta, quality, margin


def carrier_estimate(iq, samplerate, symrate, oqpsk, starts, window_samples, chirp=None, round_seq=False, round_mags=False):
    """carrier_line_kernel in float64, one dict per window: k, delta (the line sits at k + delta bins), quality, margin, and
    freq = (k + delta) * samplerate / nwin / 4 in rad per NCO step.  round_seq / round_mags put the float32 roundings in that
    the tests measure their tolerance with."""
    nwin, decim, l2, kmax, pre = carrier_geometry(samplerate, symrate, window_samples)
    nf = 1 << l2
    x = to_float(iq)
    nco = 2 if oqpsk else 1
    hz_per_bin_over4 = float(samplerate) / nwin / 4.0
    rad_per_hz = 2 * math.pi / (float(symrate) * nco)
    # the entry hands the kernel float32 words: the slope and its scale are multiplied as such
    chirp_scale = np.float32(nco * float(symrate) / float(samplerate) / math.pi)
    out = []
    for w, s0 in enumerate(starts):
        z = _window_samples(x, s0, nwin)
        z = z - z.mean()                                            # 1. mean removal
        v = z.reshape(nwin // pre, pre).sum(axis=1)                 # 2. sums of `pre` samples
        z4 = v ** 4                                                 # 3. the 4th power
        c4 = float(np.float32(chirp[w]) * chirp_scale) if chirp is not None else 0.0
        if c4 != 0.0:                                               # 4. de-chirp around the middle of the window
            t = np.arange(nwin // pre) * pre + 0.5 * (pre - 1) - 0.5 * nwin
            z4 = z4 * np.exp(2j * np.pi * (-c4 * t * t))
        seq = z4.reshape(nf, decim // pre).sum(axis=1)              # 5. boxcar over decim
        seq = seq * _hann(nf) * (1e-12 / pre ** 4)                  # 6. Hann window (and the kernel's overflow guard)
        if round_seq:
            seq = seq.astype(np.complex64).astype(np.complex128)
        spec = np.fft.fft(seq)                                      # 7.
        k, delta, quality, margin = _peak(spec, kmax, kmax, round_mags)      # 8. - 10.
        out.append(dict(k=k, delta=delta, quality=quality, margin=margin, freq=(k + delta) * hz_per_bin_over4 * rad_per_hz,
                        nwin=nwin, decim=decim, log2_nf=l2, kmax=kmax, pre=pre))
    return out


def clock_estimate(iq, samplerate, symrate, oqpsk, interp, starts, window_samples, carrier=None, chirp=None, round_seq=False, round_mags=False):
    """clock_line_kernel in float64, one dict per window: per line k and delta, pos = the deviation from the nominal rate in
    bins of the window (QPSK: the line's position; OQPSK: half the distance of the two lines), quality, margin and
    t_freq = (f_nom + pos / nwin) * 2 pi / interp."""
    nwin, decim, l2, kmax, knoise = clock_geometry(samplerate, symrate, oqpsk, window_samples)
    nf = 1 << l2
    x = to_float(iq)
    nco = 2 if oqpsk else 1
    f_nom = float(symrate) / float(samplerate)
    carrier_scale = float(symrate) * nco / float(samplerate) / (2 * math.pi)
    chirp_scale = nco * float(symrate) / float(samplerate) / (2 * math.pi)
    n = np.arange(nwin, dtype=np.float64)
    out = []
    for w, s0 in enumerate(starts):
        z = _window_samples(x, s0, nwin)
        if oqpsk:
            u = z * z
            c2 = float(chirp[w]) * chirp_scale if chirp is not None else 0.0
            if c2 != 0.0:
                t = n - 0.5 * nwin
                u = u * np.exp(2j * np.pi * (-c2 * t * t))
            fc2 = 2.0 * float(carrier[w]) * carrier_scale if carrier is not None else 0.0
            lines = [fc2 + f_nom, fc2 - f_nom]
        else:
            u = (np.abs(z) ** 2).astype(np.complex128)
            lines = [f_nom]
        res = []
        for fl in lines:
            ph = n * fl
            seq = (u * np.exp(-2j * np.pi * (ph - np.floor(ph)))).reshape(nf, decim).sum(axis=1) * _hann(nf)
            if round_seq:
                seq = seq.astype(np.complex64).astype(np.complex128)
            res.append(_peak(np.fft.fft(seq), kmax, knoise, round_mags))
        p = [r[0] + r[1] for r in res]
        pos = 0.5 * (p[0] - p[1]) if oqpsk else p[0]
        out.append(dict(k=[r[0] for r in res], delta=[r[1] for r in res], pos=pos, quality=min(r[2] for r in res),
                        margin=min(r[3] for r in res), t_freq=(f_nom + pos / nwin) * 2 * math.pi / interp,
                        nwin=nwin, decim=decim, kmax=kmax, knoise=knoise))
    return out
