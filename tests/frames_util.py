"""Signals for the frame layer's tests (test_frames_host.py, test_gpu_frames.py): a numpy encoder, framed streams of soft symbols
through the eight hypotheses, and one modulated recording.  Everything is seeded; what is expensive is made once per process."""
from __future__ import annotations

import functools

import numpy as np

MARKER = bytes([0x1A, 0xCF, 0xFC, 0x1D])
FRAME = 8192
AMP = 48.0


def encode(bits: np.ndarray, history: np.ndarray | None = None) -> np.ndarray:
    """The rate-1/2 K = 7 encoder in numpy: bits (0 / 1) -> [n, 2] of (c1, c2) as 0 / 1.  reg = ((reg << 1) | bit) & 0x7F, so bit j of
    the register is the input j steps ago; c1 = parity(reg & 0x4F) taps 0, 1, 2, 3, 6 and c2 = parity(reg & 0x6D) taps 0, 2, 3, 5, 6.
    `history`: the six bits before (zeros: the zero state)."""
    h = np.zeros(6, dtype=np.uint8) if history is None else np.asarray(history, dtype=np.uint8)
    x = np.concatenate([h, np.asarray(bits, dtype=np.uint8)])
    n = len(bits)
    tap = lambda j: x[6 - j: 6 - j + n]                                      # noqa: E731
    c1 = tap(0) ^ tap(1) ^ tap(2) ^ tap(3) ^ tap(6)
    c2 = tap(0) ^ tap(2) ^ tap(3) ^ tap(5) ^ tap(6)
    return np.stack([c1, c2], axis=1)


def word_of(sym01: np.ndarray, swap: bool = False, invert: bool = False) -> int:
    """The symbols' bits as one integer, c1 first (c2 first when the rails are swapped)."""
    s = sym01[:, ::-1] if swap else sym01
    v = 0
    for b in s.reshape(-1):
        v = (v << 1) | int(b ^ invert)
    return v


def through_inverse(sym: np.ndarray, h: int) -> np.ndarray:
    """What must be received so that hypothesis h reads `sym` ([n, 2], any sign convention)."""
    i, q = sym[:, 0], sym[:, 1]
    out = {0: (i, q), 1: (q, -i), 2: (-i, -q), 3: (-q, i), 4: (i, -q), 5: (q, i), 6: (-i, q), 7: (-q, -i)}[h]
    return np.stack(out, axis=1)


def through(soft: np.ndarray, h: int) -> np.ndarray:
    """Hypothesis h of the issue's table, in int32."""
    i, q = soft[:, 0].astype(np.int32), soft[:, 1].astype(np.int32)
    out = {0: (i, q), 1: (-q, i), 2: (-i, -q), 3: (q, -i), 4: (i, -q), 5: (q, i), 6: (-i, q), 7: (-q, -i)}[h]
    return np.stack(out, axis=1)


def sigma_of(esn0_db: float) -> float:
    """Es = 2 AMP^2 (both rails), N0 / 2 = sigma^2 per rail: Es / N0 = AMP^2 / sigma^2."""
    return AMP / np.sqrt(10 ** (esn0_db / 10))


def quantise(x: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(x), -128, 127).astype(np.int8)


class Stream:
    """n_frames frames (marker + 1020 random bytes) between `lead` and `tail` random bits, encoded without a reset."""

    def __init__(self, seed: int, n_frames: int = 5, lead: int = 777, tail: int = 300):
        rng = np.random.default_rng(seed)
        self.lead, self.n_frames = lead, n_frames
        self.frames = [MARKER + rng.integers(0, 256, 1020, dtype=np.uint8).tobytes() for _ in range(n_frames)]
        bits = [rng.integers(0, 2, lead, dtype=np.uint8)]
        bits += [np.unpackbits(np.frombuffer(f, dtype=np.uint8)) for f in self.frames]
        bits += [rng.integers(0, 2, tail, dtype=np.uint8)]
        self.bits = np.concatenate(bits)
        self.sym = encode(self.bits).astype(np.float64) * 2 - 1                # [m, 2] of +-1
        self.positions = [lead + FRAME * k for k in range(n_frames)]

    def received(self, h, esn0_db: float, seed: int) -> np.ndarray:
        """int8 [m, 2]: amplitude 48, Gaussian noise, rounded and clipped, sent through the inverse of hypothesis h (an int, or an
        array with one h per symbol)."""
        rng = np.random.default_rng(seed)
        if np.isscalar(h):
            x = through_inverse(self.sym, int(h))
        else:
            x = np.empty_like(self.sym)
            for v in np.unique(h):
                x[h == v] = through_inverse(self.sym, int(v))[h == v]
        return quantise(AMP * x + sigma_of(esn0_db) * rng.normal(size=x.shape))


def noise(m: int, seed: int, sigma: float = 40.0) -> np.ndarray:
    return quantise(sigma * np.random.default_rng(seed).normal(size=(m, 2)))


def hard_error_rate(soft: np.ndarray, h: int, st: Stream) -> float:
    """The share of hard decisions of the input (through h) that differ from what was sent."""
    return float(((through(soft, h) > 0) != (st.sym > 0)).mean())


# ---------------------------------------------------------------------------------------------------------- the recording
SPS = 4
REC_SAMPLERATE = 72000 * SPS
REC_FRAMES = 9


def _rrc(alpha: float, sps: int, span: int) -> np.ndarray:
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


@functools.lru_cache(maxsize=1)
def recording():
    """(Stream, s16 [n, 2]): REC_FRAMES frames as QPSK, RRC 0.6, 4 samples per symbol, carrier at 0 Hz, Es/N0 about 13 dB."""
    st = Stream(seed=4242, n_frames=REC_FRAMES, lead=3000, tail=600)
    rng = np.random.default_rng(77)
    z = np.zeros(len(st.sym) * SPS, dtype=complex)
    z[::SPS] = st.sym[:, 0] + 1j * st.sym[:, 1]
    y = np.convolve(z, _rrc(0.6, SPS, 8))                                     # unit-energy pulse: Es = 2
    y = y + np.sqrt(2 / 10 ** 1.3 / 2) * (rng.normal(size=len(y)) + 1j * rng.normal(size=len(y)))
    iq = np.stack([y.real, y.imag], axis=1) * 4000.0
    return st, np.clip(np.rint(iq), -32768, 32767).astype(np.int16)


def recording_cfg():
    from meteor_demod_amd import DemodConfig
    return DemodConfig(samplerate=REC_SAMPLERATE, bps=16)


@functools.lru_cache(maxsize=1)
def recording_cpu():
    """The recording through the CPU demodulator and the host model: (soft, first lock symbol, CADUs, frames)."""
    import oracle_py
    from meteor_demod_amd import frames
    _, iq = recording()
    soft, _, events = oracle_py.oracle_demod(recording_cfg(), iq)
    lock = next(s for s, locked in events if locked)
    cadu, fr = frames.model_decode(soft)
    return soft, lock, cadu, fr


def wav_bytes(fs: int, samples: np.ndarray) -> bytes:
    import struct
    data = samples.astype("<i2").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, fs, fs * 4, 4, 16)
    return hdr + b"data" + struct.pack("<I", len(data)) + data
