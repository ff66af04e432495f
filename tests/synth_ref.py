"""An independent reference of the synthetic source (csrc/synth_core.h) and of the truth counts (csrc/synth.hip), written from the
header's text and the signal model.  It never calls the library: time bases are Python integers (unbounded, so no product wraps),
the pulse is the closed-form root-raised cosine in float64 (no table, no interpolation), the carrier is math.cos / math.sin of
the full 32-bit phase word, and the truth counts are plain numpy compares.  Stream descriptors are read by attribute only, so
anything with the fields of synth.SynthStream will do.

Used by tests/test_synth_host.py (CPU: host generator == this model) and tests/test_gpu_synth.py (GPU: device generator == host
generator bit for bit; truth kernels == these counts exactly)."""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
NOISE_MUL = 0xD1B54A32D192ED03
SALT_I, SALT_Q = 0x1234567, 0x89ABCDE
SPAN = 6
ALPHA = 0.6


# ---- hash, symbols, noise ------------------------------------------------------------------------------------------------------

def mix64(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def mix64_np(z) -> np.ndarray:
    """mix64 on a numpy.uint64 array (multiplication wraps modulo 2^64 by itself)."""
    z = np.array(z, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def symbol(seed: int, j: int) -> tuple[int, int]:
    """(+-1, +-1): the I and the Q rail of transmitted symbol j."""
    h = mix64(seed + (j + 1) * GOLD)
    return (1 if h & 1 else -1), (1 if h & 2 else -1)


def symbols_np(seed: int, j) -> tuple[np.ndarray, np.ndarray]:
    """symbol() for a numpy array of symbol numbers (taken modulo 2^64): two int8 arrays of +-1."""
    j = np.asarray(j).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = mix64_np(np.uint64(seed & M64) + (j + np.uint64(1)) * np.uint64(GOLD))
    si = np.where(h & np.uint64(1), 1, -1).astype(np.int8)
    sq = np.where(h & np.uint64(2), 1, -1).astype(np.int8)
    return si, sq


def noise(seed: int, n: int, salt: int) -> float:
    """Zero-mean sum of eight 16-bit uniforms (the halves of two hashes), in units of one: an integer or a half."""
    h1 = mix64(seed ^ ((salt + n * NOISE_MUL) & M64))
    h2 = mix64(h1 + GOLD)
    s = sum((h >> (16 * i)) & 0xFFFF for h in (h1, h2) for i in range(4))
    return (2 * s - 8 * 65535) * 0.5


# ---- the signal model ----------------------------------------------------------------------------------------------------------

def rrc(t, alpha: float = ALPHA) -> np.ndarray:
    """Unit-energy root-raised cosine (symbol period 1), closed form, float64, for an array of times in symbols."""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    x = 4.0 * alpha * t
    zero = np.abs(t) < 1e-12
    pole = np.abs(np.abs(x) - 1.0) < 1e-9
    ts = np.where(zero | pole, 0.25, t)              # any harmless point; overwritten below
    xs = 4.0 * alpha * ts
    out = (np.sin(np.pi * ts * (1 - alpha)) + xs * np.cos(np.pi * ts * (1 + alpha))) / (np.pi * ts * (1 - xs * xs))
    out = np.where(zero, 1.0 - alpha + 4.0 * alpha / np.pi, out)
    at_pole = alpha / math.sqrt(2.0) * ((1 + 2 / np.pi) * math.sin(np.pi / (4 * alpha)) + (1 - 2 / np.pi) * math.cos(np.pi / (4 * alpha)))
    return np.where(pole, at_pole, out)


def time_bases(st, n: int) -> tuple[int, int]:
    """(symbol time t as 32.32 modulo 2^64, carrier phase as 2^-32 turns modulo 2^32) of sample n, with the exact triangle."""
    tri = n * (n - 1) // 2
    t = (st.sym_phase0 + n * st.sym_step + ((tri * st.clk_ramp64) >> 32)) & M64
    th = (st.car_phase0 + n * st.car_step + ((tri * st.car_ramp48) >> 16)) & 0xFFFFFFFF
    return t, th


def _rail(seed: int, t: int, rail: int) -> float:
    k, frac = t >> 32, (t & 0xFFFFFFFF) / 4294967296.0
    acc = 0.0
    for m in range(-SPAN + 1, SPAN + 1):
        acc += symbol(seed, (k + m) & M64)[rail] * float(rrc(frac - m)[0])
    return acc


def baseband(st, n: int) -> complex:
    """The unit-amplitude rails of sample n before the carrier: I + jQ, Q half a symbol late for OQPSK."""
    t, _ = time_bases(st, n)
    return complex(_rail(st.seed, t, 0), _rail(st.seed, (t - (1 << 31)) & M64 if st.oqpsk else t, 1))


def ideal_sample(st, n: int) -> tuple[float, float]:
    """Sample n of the stream as real (I, Q) before quantisation, by the signal model."""
    _, th = time_bases(st, n)
    b = baseband(st, n)
    ang = 2.0 * math.pi * th / 4294967296.0
    c, s = math.cos(ang), math.sin(ang)
    ri, rq = b.real * c - b.imag * s, b.real * s + b.imag * c
    return (st.amp * ri + st.dc_i + st.noise_scale * noise(st.seed, n, SALT_I),
            st.amp * rq + st.dc_q + st.noise_scale * noise(st.seed, n, SALT_Q))


def _rails_np(seed: int, ts: list[int], rail: int) -> np.ndarray:
    k = np.array([t >> 32 for t in ts], dtype=np.uint64)
    frac = np.array([t & 0xFFFFFFFF for t in ts], dtype=np.float64) / 4294967296.0
    acc = np.zeros(len(ts))
    for m in range(-SPAN + 1, SPAN + 1):
        with np.errstate(over="ignore"):
            j = k + np.uint64(m & M64)
        acc += symbols_np(seed, j)[rail] * rrc(frac - m)
    return acc


def ideal_samples(st, n0: int, count: int, with_noise: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """(samples, baseband) of [n0, n0 + count) as complex128 arrays: ideal_sample() with the symbol sums vectorised.  The time
    bases stay Python integers."""
    tb = [time_bases(st, n0 + i) for i in range(count)]
    ts = [t for t, _ in tb]
    bi = _rails_np(st.seed, ts, 0)
    bq = _rails_np(st.seed, [(t - (1 << 31)) & M64 for t in ts] if st.oqpsk else ts, 1)
    ang = np.array([2.0 * math.pi * th / 4294967296.0 for _, th in tb])
    c, s = np.cos(ang), np.sin(ang)
    oi = st.amp * (bi * c - bq * s) + st.dc_i
    oq = st.amp * (bi * s + bq * c) + st.dc_q
    if with_noise and st.noise_scale:
        oi = oi + st.noise_scale * np.array([noise(st.seed, n0 + i, SALT_I) for i in range(count)])
        oq = oq + st.noise_scale * np.array([noise(st.seed, n0 + i, SALT_Q) for i in range(count)])
    return oi + 1j * oq, bi + 1j * bq


def interpolation_bound(os: int = 256, alpha: float = ALPHA) -> float:
    """Largest error of one rail built from a pulse table of `os` points per symbol read with linear interpolation: over each
    tap's unit interval the error of a chord is at most h^2 / 8 * max |rrc''|, and the 2 * SPAN taps (symbols of magnitude 1) can
    at worst add up.  rrc'' is a central second difference of the closed form."""
    h, e, grid = 1.0 / os, 1e-3, 4096
    total = 0.0
    for m in range(-SPAN + 1, SPAN + 1):
        tau = -m + np.arange(grid + 1) / grid
        d2 = (rrc(tau + e, alpha) - 2.0 * rrc(tau, alpha) + rrc(tau - e, alpha)) / (e * e)
        total += h * h / 8.0 * float(np.abs(d2).max())
    return total


# ---- truth counts --------------------------------------------------------------------------------------------------------------

def _decisions(soft) -> tuple[np.ndarray, np.ndarray]:
    soft = np.asarray(soft).view(np.int8).reshape(-1, 2)
    return soft[:, 0] >= 0, soft[:, 1] >= 0


def probe_counts(seed: int, soft, m0: int, count: int, lag_min: int, n_lags: int) -> np.ndarray:
    """uint32 [2, 2, n_lags]: [r, t, l] = symbols m of [m0, m0 + count) on which the decision of received rail r (0 is positive)
    equals transmitted rail t of symbol m + lag_min + l.  Symbols before the first transmitted one (m + lag < 0) are skipped."""
    ri, rq = _decisions(soft)
    rx = (ri[m0:m0 + count], rq[m0:m0 + count])
    out = np.zeros((2, 2, n_lags), dtype=np.uint32)
    j = m0 + lag_min + np.arange(count + n_lags - 1, dtype=np.int64)         # every transmitted symbol any lag looks at
    sent = j >= 0
    si, sq = symbols_np(seed, np.where(sent, j, 0))
    for l in range(n_lags):
        ok = sent[l:l + count]
        tx = (si[l:l + count] > 0, sq[l:l + count] > 0)
        for r in range(2):
            for t in range(2):
                out[r, t, l] = np.count_nonzero((rx[r] == tx[t]) & ok)
    return out


def error_counts(seed: int, soft, n_symbols: int, block: int, hyp) -> tuple[np.ndarray, np.ndarray]:
    """(err_i, err_q), one entry per block of `block` symbols: decisions of the received I (Q) rail that differ from transmitted
    rail hyp[0] (hyp[3]) of symbol m + hyp[1] (m + hyp[4]), inverted where hyp[2] (hyp[5]).  m + lag < 0 is skipped."""
    rx = _decisions(soft)
    nb = (n_symbols + block - 1) // block
    out = []
    m = np.arange(n_symbols, dtype=np.int64)
    for r in range(2):
        rail, lag, inv = hyp[3 * r:3 * r + 3]
        j = m + lag
        ok = j >= 0
        tx = (symbols_np(seed, np.where(ok, j, 0))[rail] > 0) != bool(inv)
        wrong = (rx[r][:n_symbols] != tx) & ok
        e = np.zeros(nb, dtype=np.uint32)
        for b in range(nb):
            e[b] = np.count_nonzero(wrong[b * block:(b + 1) * block])
        out.append(e)
    return out[0], out[1]


# ---- soft arrays with a known relation to the transmitted symbols --------------------------------------------------------------

POSITIVE, NEGATIVE = np.array([0, 1, 127], dtype=np.int8), np.array([-1, -128], dtype=np.int8)


def _magnitudes(positive: np.ndarray, rng) -> np.ndarray:
    return np.where(positive, POSITIVE[rng.integers(0, 3, positive.shape)], NEGATIVE[rng.integers(0, 2, positive.shape)]).astype(np.int8)


def soft_from(seed: int, m: int, rail_i: int, lag_i: int, inv_i: int, rail_q: int, lag_q: int, inv_q: int, magnitudes=0) -> np.ndarray:
    """int8 [m, 2] whose decisions are the transmitted symbols under the pairing "received I = transmitted rail_i of symbol
    m + lag_i, inverted if inv_i", and the same for Q.  `magnitudes` seeds the draw of the values: 0, 1 or 127 for a positive
    decision (0 counts as positive), -1 or -128 for a negative one.  Symbols before the first transmitted one decide positive."""
    rng = np.random.default_rng(magnitudes)
    out = np.empty((m, 2), dtype=np.int8)
    idx = np.arange(m, dtype=np.int64)
    for r, (rail, lag, inv) in enumerate(((rail_i, lag_i, inv_i), (rail_q, lag_q, inv_q))):
        j = idx + lag
        pos = (symbols_np(seed, np.where(j >= 0, j, 0))[rail] > 0) != bool(inv)
        out[:, r] = _magnitudes(pos | (j < 0), rng)
    return out


def flip(soft: np.ndarray, symbols, rail: int) -> np.ndarray:
    """Copy with the decision of `rail` turned round at the given symbols (0 -> -1, 1 -> -128, 127 -> -1, -1 -> 0, -128 -> 127)."""
    out = soft.copy()
    s = np.asarray(symbols, dtype=np.int64)
    v = out[s, rail].astype(np.int16)
    out[s, rail] = np.where(v >= 0, np.where(v == 1, -128, -1), np.where(v == -128, 127, 0)).astype(np.int8)
    return out


def rotate_from(seed: int, soft: np.ndarray, start: int, rail_i: int, lag_i: int, inv_i: int, rail_q: int, lag_q: int, inv_q: int) -> np.ndarray:
    """Copy in which the loop turns by +90 degrees from symbol `start` on: there the received I rail is the earlier Q rail
    inverted and the received Q rail the earlier I rail.  The arguments are the pairing BEFORE the turn."""
    out = soft.copy()
    tail = soft_from(seed, soft.shape[0], rail_q, lag_q, 1 - inv_q, rail_i, lag_i, inv_i, magnitudes=start)
    out[start:] = tail[start:]
    return out


def delete_symbol(soft: np.ndarray, at: int) -> np.ndarray:
    """Copy without symbol `at` (one symbol shorter): from there on every lag is one more."""
    return np.delete(soft, at, axis=0)


def randomise(soft: np.ndarray, start: int, stop: int, seed: int) -> np.ndarray:
    """Copy with symbols [start, stop) overwritten by seeded random bytes."""
    out = soft.copy()
    out[start:stop] = np.random.default_rng(seed).integers(-128, 128, (stop - start, 2), dtype=np.int8)
    return out
