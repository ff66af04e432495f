"""Inputs of the stitcher kernel tests: planted seam pairs and the batches made of them, and the estimator cases.  numpy only;
what the answers are is stitch_ref's business, not this file's."""
from __future__ import annotations

import math

import numpy as np

from stitch_ref import rot_sym

MODES = ("tails", "rails", "heads")
SHIFT_ROT = [(s, r) for s in (0, 1, -1) for r in range(4)]


def _rot(x, k):
    i, q = rot_sym(x[:, 0], x[:, 1], k)
    return np.stack((i, q), axis=1)


def _base(rng, n, amp=None):
    """QPSK-like symbols: random signs, magnitudes 40..100 (or `amp` everywhere)."""
    mag = rng.integers(40, 101, size=(n, 2)) if amp is None else np.full((n, 2), amp)
    return mag * rng.choice([-1, 1], size=(n, 2))


def _noisy(rng, x, noise):
    return np.clip(x + rng.integers(-noise, noise + 1, size=x.shape), -127, 127) if noise else x


def planted(mode, rng, K, s, r, a_cnt, b_cnt, noise=10, amp=None, b_rot=0, d_i=0, d_q=0):
    """A pair whose B is A turned by -r quarter turns and displaced so that the match of `mode` answers (s, r) (rails: r, with
    the I and Q rails of B * j^r found at shifts d_i and d_q), plus uniform noise of +-`noise`; B is stored turned back by b_rot.
    Tails are aligned at their ends, heads at their starts."""
    n = max(a_cnt, b_cnt) + 4
    base = _base(rng, n, amp)
    if mode == 0:
        a, b = base[1:1 + a_cnt][::-1], _rot(base[1 + s:1 + s + b_cnt], -r)[::-1]
    elif mode == 2:
        a, b = base[1:1 + a_cnt], _rot(base[1 + s:1 + s + b_cnt], -r)
    else:
        m = np.stack((base[1 + d_i:1 + d_i + b_cnt, 0], base[1 + d_q:1 + d_q + b_cnt, 1]), axis=1)
        a, b = base[1:1 + a_cnt][::-1], _rot(m, -r)[::-1]
    return dict(a=np.ascontiguousarray(a), b=np.ascontiguousarray(_rot(_noisy(rng, b, noise), -b_rot)), b_rot=b_rot, force_weak=0)


def _sparse(cnt, at_end, pos, val):
    """Zeros but for `val` at the positions `pos`, counted from the end (tails) or the start (heads)."""
    x = np.zeros((cnt, 2), dtype=np.int64)
    for p in pos:
        x[cnt - 1 - p if at_end else p] = val
    return x


def seam_batch(mode, K, seed=0):
    """About 200 pairs of every kind a seam match can meet (see tests/test_gpu_stitch_kernels.py for the list), ordered so that
    neighbours differ in kind.  Every pair is a dict a, b (int [cnt, 2]), b_rot, force_weak, kind."""
    rng = np.random.default_rng(1000 * mode + K + seed)
    tail = K + 2 if mode == 1 else K + 1
    full = (K + 8, K + 11)
    kinds: dict[str, list] = {}

    def add(kind, p, **kw):
        p = dict(p, kind=kind, **kw)
        kinds.setdefault(kind, []).append(p)

    combos = [(0, r, d, d) for r in range(4) for d in (-1, 0, 1)] if mode == 1 else [(s, r, 0, 0) for s, r in SHIFT_ROT]
    for j, (s, r, di, dq) in enumerate(combos):
        add("planted", planted(mode, rng, K, s, r, *full, d_i=di, d_q=dq), want=(s, r, di))
        add("planted_exact_tail", planted(mode, rng, K, s, r, *((tail, K + 9) if j % 2 else (K + 9, tail)), d_i=di, d_q=dq))
        add("full_scale", planted(mode, rng, K, s, r, *full, noise=0, amp=127, d_i=di, d_q=dq))
        add("b_rot", planted(mode, rng, K, s, r, *full, b_rot=(j % 4) if mode == 0 else 0, d_i=di, d_q=dq))
        add("forced", planted(mode, rng, K, s, r, *full, d_i=di, d_q=dq), force_weak=1)
    if mode == 1:
        for r in range(4):                                        # the two rails paired at different shifts
            for di, dq in ((-1, 1), (1, 0), (0, -1)):
                add("planted", planted(mode, rng, K, 0, r, *full, d_i=di, d_q=dq))
    counts = [(K, K + 8), (K + 8, K), (1, K + 8), (K + 8, 1), (0, K + 8), (K + 8, 0), (0, 0), (1, 1), (K // 2, K + 8), (K + 8, K // 2), (tail, tail)]
    for j, (ca, cb) in enumerate(counts):
        for s, r, di, dq in (combos[j % 12], combos[(5 * j + 3) % 12]):
            add("counts", planted(mode, rng, K, s, r, ca, cb, d_i=di, d_q=dq))
    for j in range(8):                                            # unrelated: weak by the energy rule
        add("unrelated", dict(a=_base(rng, K + 8), b=_base(rng, K + 9), b_rot=0, force_weak=0))
    z = lambda n: np.zeros((n, 2), dtype=np.int64)
    add("zeros", dict(a=z(K + 8), b=z(K + 8), b_rot=0, force_weak=0))
    add("zeros", dict(a=z(K + 8), b=_base(rng, K + 8), b_rot=0, force_weak=0))
    add("zeros", dict(a=_base(rng, K + 8), b=z(K + 9), b_rot=0, force_weak=0))
    add("zeros", planted(mode, rng, K, 0, 2, *full, noise=0, d_i=0, d_q=0))       # anti-correlated under rot 0 only: still matches at rot 2
    # exact ties.  Between shifts: a constant symbol looks the same at every shift.  Between rotations: a * conj(b) on a diagonal
    # (tails, heads), or one rail of b empty (rails).
    for j, (av, bv) in enumerate([((50, 0), (50, 0)), ((50, 0), (0, 50)), ((30, -40), (-30, 40)), ((0, 60), (60, 0)),
                                  ((50, 0), (50, -50)), ((50, 0), (-50, -50)), ((50, 50), (50, 0)), ((50, 50), (0, 50)),
                                  ((50, 50), (-50, 0)), ((50, 50), (0, -50)), ((20, 70), (70, -20)), ((50, 0), (50, 50))]):
        add("ties", dict(a=np.tile(av, (K + 8, 1)), b=np.tile(bv, (K + 8 + j % 3, 1)), b_rot=0, force_weak=0))
    uv = np.array([(36, 77), (-51, 68)])                           # period 2 (both of energy 85^2), b one symbol on: shifts +1 and -1 both fit perfectly
    add("ties", dict(a=np.tile(uv, (K // 2 + 5, 1)), b=np.tile(uv[::-1], (K // 2 + 5, 1)), b_rot=0, force_weak=0))
    # the weak boundary: a and b sparse with ma, mb symbols of (p, 0) and (q, 0), mo of them on the same place: best = p q mo,
    # Ea Eb = p^2 q^2 ma mb, so 4 best^2 == Ea Eb for (mo, ma, mb) = (2, 4, 4), (1, 2, 2), (3, 6, 6); one more count in Ea tips it.
    for p, q, pa, pb in ((100, 90, (5, 9, 13, 17), (5, 9, 21, 25)), (127, 127, (4, 8), (4, 12)), (-77, -13, (3, 6, 9, 12, 15, 18), (3, 6, 9, 21, 24, 27))):
        for extra in (0, 1):
            a = _sparse(K + 8, mode != 2, pa, (p, 0))
            b = _sparse(K + 10, mode != 2, pb, (q, 0))
            if extra:
                a[(K + 8 - 1 - 20) if mode != 2 else 20] += (0, 1)
            add("boundary_below" if extra else "boundary", dict(a=a, b=b, b_rot=0, force_weak=0))
    j = 0
    while sum(len(v) for v in kinds.values()) < 200:              # filler: random answers, random noise, random counts
        s, r, di, dq = combos[int(rng.integers(len(combos)))]
        add("random", planted(mode, rng, K, s, r, int(rng.integers(tail, K + 40)), int(rng.integers(tail, K + 40)), noise=int(rng.integers(0, 60)),
                              b_rot=int(rng.integers(4)) if mode == 0 else 0, d_i=di, d_q=dq), force_weak=int(j % 7 == 3))
        j += 1
    order, lists = [], [list(v) for v in kinds.values()]
    while any(lists):                                             # round robin over the kinds
        for l in lists:
            if l:
                order.append(l.pop(0))
    return order


def pack(pairs, key):
    """All arrays `key` of the pairs in one int8 buffer [n, 2], one symbol of padding (99, -99) in front of each (offsets of both
    parities): (buffer, offsets, counts)."""
    parts, off, cnt, at = [], [], [], 0
    for j, p in enumerate(pairs):
        pad = 1 + (j % 2)
        parts.append(np.tile((99, -99), (pad, 1)))
        at += pad
        off.append(at)
        cnt.append(len(p[key]))
        parts.append(np.asarray(p[key]).reshape(-1, 2))
        at += len(p[key])
    parts.append(np.tile((99, -99), (8, 1)))
    buf = np.concatenate(parts).astype(np.int64)
    assert buf.min() >= -128 and buf.max() <= 127
    return buf.astype(np.int8), np.array(off, dtype=np.uint64), np.array(cnt, dtype=np.uint32)


# ---- estimator cases ---------------------------------------------------------------------------------------------------------

AMP = {8: dict(rms=40.0, dc=(1.5, -1.0)), 16: dict(rms=3000.0), 32: dict(rms=0.25, dc=(0.001, -0.002))}
# the recording's last sample, which every read past the end repeats: a constant whose sums are exact in float32 (carrier: the
# mean comes out exact and the window past the end is all zero after the mean removal), resp. zero itself (clock: no mean removal)
LAST_CARRIER = {8: (160, 112), 16: (64, -32), 32: (0.25, -0.125)}
LAST_CLOCK = {8: (128, 128), 16: (0, 0), 32: (0.0, 0.0)}

# name: samplerate, symrate, oqpsk, bps, window, (decim, pre) the case is there for, f0 Hz, ramp Hz/s (0: no de-chirp), seed
CARRIER_CASES = {
    "s16_230k_w4096": (230000, 72000, False, 16, 4096, (1, 1), -437.0, 0.0, 1),
    "s16_230k_w65536": (230000, 72000, False, 16, 65536, (4, 1), 311.0, 0.0, 1),
    "u8_1M_w8192": (1000000, 72000, False, 8, 8192, (2, 2), 1234.0, 0.0, 1),
    "f32_1M_w65536": (1000000, 72000, False, 32, 65536, (16, 4), -780.0, 0.0, 1),
    "oqpsk_s16_1024k_chirp": (1024000, 80000, True, 16, 65536, (16, 4), 520.0, 1024000.0 ** 2 / 2.0 ** 48, 1),
    "s16_72k_one_sample_per_symbol": (72000, 72000, False, 16, 65536, (1, 1), 95.0, 0.0, 1),
}
# name: samplerate, symrate, oqpsk, bps, window, decim, f0 Hz, ramp Hz/s, clock ppm, seed
CLOCK_CASES = {
    "qpsk_w4096": (230000, 72000, False, 16, 4096, 1, 900.0, 0.0, 7.3, 1),
    "oqpsk_w4096": (230000, 80000, True, 16, 4096, 1, 900.0, 0.0, 31.0, 1),
    "qpsk_w65536": (230000, 72000, False, 16, 65536, 16, 900.0, 0.0, -150.0, 1),
    "oqpsk_w65536": (230000, 80000, True, 16, 65536, 16, -600.0, 0.0, 31.0, 1),
    "qpsk_u8_w262144": (230000, 72000, False, 8, 262144, 64, 900.0, 0.0, 40.0, 1),
    "oqpsk_f32_w262144": (230000, 80000, True, 32, 262144, 64, 300.0, 0.0, -12.0, 1),
    "oqpsk_carrier_chirp_w65536": (230000, 80000, True, 16, 65536, 16, 900.0, 40.0, 12.0, 1),
}
N_RECORDING = 300_000


def estimator_windows(nwin):
    """Inside the recording (odd start), half over its end, wholly past it."""
    return np.array([1001, N_RECORDING - nwin // 2, N_RECORDING + 5], dtype=np.int64)


def make_recording(synth, samplerate, symrate, oqpsk, bps, f0, ramp, ppm, seed, last):
    st = synth.make_stream(seed, samplerate, symrate, f0_hz=f0, clock_ppm=ppm, esn0_db=12.0, oqpsk=oqpsk, fmt=bps, doppler_hz_per_s=ramp, **AMP[bps])
    iq = synth.generate_host(st, N_RECORDING)
    iq[-1] = last[bps]
    return st, iq


def carrier_inputs(synth, name):
    """(iq, starts, chirp or None, nwin-independent arguments of stitch_ref.carrier_estimate) of a carrier case."""
    fs, sr, oq, bps, window, _, f0, ramp, seed = CARRIER_CASES[name]
    _, iq = make_recording(synth, fs, sr, oq, bps, f0, ramp, 3.0, seed, LAST_CARRIER)
    nco = 2 if oq else 1
    chirp = np.full(3, 2 * math.pi * ramp / (sr * nco) / fs, dtype=np.float32) if ramp else None      # rad per NCO step per sample
    return iq, chirp


def clock_inputs(synth, name, nwin):
    fs, sr, oq, bps, window, _, f0, ramp, ppm, seed = CLOCK_CASES[name]
    st, iq = make_recording(synth, fs, sr, oq, bps, f0, ramp, ppm, seed, LAST_CLOCK)
    nco = 2 if oq else 1
    starts = estimator_windows(nwin)
    carrier = (2 * math.pi * (f0 + ramp * (starts + nwin // 2) / fs) / (sr * nco)).astype(np.float32) if oq else None
    chirp = np.full(3, 2 * math.pi * ramp / (sr * nco) / fs, dtype=np.float32) if (oq and ramp) else None
    return st, iq, carrier, chirp
