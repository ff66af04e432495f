"""Signals for the tests of the frame layer's link variant (test_frames_link_host.py, test_gpu_frames_link.py): an NRZ-M sender in
front of frames_util's encoder, the skew operator (what must be received so that the combined hypothesis H = h + 8 s reads a clean
stream), and an OQPSK recording of differentially coded frames.  Everything is seeded; what is expensive is made once per process."""
from __future__ import annotations

import functools

import numpy as np

import frames_util as U

FRAME = U.FRAME
PLAIN_H = list(range(24))
DIFF_H = [h + 8 * s for s in range(3) for h in (0, 1, 4, 5)]


def nrzm(bits: np.ndarray, before: int = 0) -> np.ndarray:
    """NRZ-M: d[t] = b[t] xor d[t-1], d[-1] = `before`."""
    return (np.cumsum(np.asarray(bits, dtype=np.int64)) + before & 1).astype(np.uint8)


def canonical(H: int, differential: bool) -> int:
    """The hypothesis the layer reports for a stream sent through the inverse of H: with `differential` the 180 degree partner
    with h in {0, 1, 4, 5}."""
    return H & ~2 if differential else H


def skew_inverse(sym: np.ndarray, H: int) -> np.ndarray:
    """What must be received ([n, 2]) so that the combined hypothesis H reads `sym`: s = 1 reads (I'[n], Q'[n+1]), so Q' is sent one
    symbol late; s = 2 reads (I'[n+1], Q'[n]), so I' is.  The late rail's first value is 0 (nothing was sent before), its last one
    falls past the end."""
    h, s = H & 7, H >> 3
    x = np.array(sym, dtype=np.float64)
    if s == 1:
        x[:, 1] = np.concatenate([[0.0], x[:-1, 1]])
    elif s == 2:
        x[:, 0] = np.concatenate([[0.0], x[:-1, 0]])
    return U.through_inverse(x, h)


class LinkStream:
    """frames_util.Stream with an NRZ-M sender: n_frames frames (marker + 1020 random bytes) between `lead` and `tail` random
    bits; with `differential` the bits pass NRZ-M (from d[-1] = `before`) ahead of the encoder."""

    def __init__(self, seed: int, n_frames: int = 5, lead: int = 777, tail: int = 300, differential: bool = False, before: int = 0):
        rng = np.random.default_rng(seed)
        self.lead, self.n_frames, self.differential = lead, n_frames, differential
        self.frames = [U.MARKER + rng.integers(0, 256, 1020, dtype=np.uint8).tobytes() for _ in range(n_frames)]
        bits = [rng.integers(0, 2, lead, dtype=np.uint8)]
        bits += [np.unpackbits(np.frombuffer(f, dtype=np.uint8)) for f in self.frames]
        bits += [rng.integers(0, 2, tail, dtype=np.uint8)]
        self.bits = np.concatenate(bits)
        self.coded = nrzm(self.bits, before) if differential else self.bits
        self.sym = U.encode(self.coded).astype(np.float64) * 2 - 1             # [m, 2] of +-1
        self.positions = [lead + FRAME * k for k in range(n_frames)]

    def received(self, H: int, esn0_db: float | None, seed: int, sign: np.ndarray | None = None) -> np.ndarray:
        """int8 [m, 2] sent through the inverse of H: amplitude 48, Gaussian noise (none for esn0_db None), rounded and clipped.
        `sign`: +-1 per symbol, a polarity the channel adds (a PLL's 180 degree slip)."""
        x = skew_inverse(self.sym, H)
        if sign is not None:
            x = x * np.asarray(sign, dtype=np.float64)[:, None]
        if esn0_db is None:
            return U.quantise(U.AMP * x)
        return U.quantise(U.AMP * x + U.sigma_of(esn0_db) * np.random.default_rng(seed).normal(size=x.shape))


# ---------------------------------------------------------------------------------------------------------- the recording
REC_SEED, REC_NOISE_SEED = 4243, 78
REC_PHASES = (0.0, 0.25, 0.5, 0.75)                                            # starting carrier phases, in turns


@functools.lru_cache(maxsize=1)
def recording_stream(rs_coded: bool = False):
    """The 9-frame NRZ-M stream of the recording.  `rs_coded`: the frames are Reed-Solomon coded, randomised transfer frames
    (rs_util), so that the transfer-frame layer can say "0 uncorrectable"."""
    st = LinkStream(seed=REC_SEED, n_frames=U.REC_FRAMES, lead=3000, tail=600, differential=True)
    if rs_coded:
        import rs_util
        from meteor_demod_amd import rs
        rng = np.random.default_rng(REC_SEED)
        st.frames = [rs.model_encode(rs_util.vcdu(rng, counter=k)).tobytes() for k in range(st.n_frames)]
        bits = st.bits.copy()
        for p, f in zip(st.positions, st.frames):
            bits[p: p + FRAME] = np.unpackbits(np.frombuffer(f, dtype=np.uint8))
        st.bits, st.coded = bits, nrzm(bits)
        st.sym = U.encode(st.coded).astype(np.float64) * 2 - 1
    return st


@functools.lru_cache(maxsize=8)
def recording(phase_turns: float = 0.0, rs_coded: bool = False):
    """(LinkStream, s16 [n, 2]): the stream as OQPSK - the Q rail two samples (half a symbol) late - RRC 0.6, 4 samples per symbol,
    carrier at 0 Hz with the given starting phase, Es/N0 about 13 dB: built like frames_util.recording."""
    st = recording_stream(rs_coded)
    rng = np.random.default_rng(REC_NOISE_SEED)
    n = len(st.sym) * U.SPS
    zi, zq = np.zeros(n + U.SPS // 2), np.zeros(n + U.SPS // 2)
    zi[: n: U.SPS] = st.sym[:, 0]
    zq[U.SPS // 2: n + U.SPS // 2: U.SPS] = st.sym[:, 1]
    pulse = U._rrc(0.6, U.SPS, 8)
    y = np.convolve(zi, pulse) + 1j * np.convolve(zq, pulse)                   # unit-energy pulse: Es = 2
    y = y + np.sqrt(2 / 10 ** 1.3 / 2) * (rng.normal(size=len(y)) + 1j * rng.normal(size=len(y)))
    y = y * np.exp(2j * np.pi * phase_turns)
    iq = np.stack([y.real, y.imag], axis=1) * 4000.0
    return st, np.clip(np.rint(iq), -32768, 32767).astype(np.int16)


def recording_cfg():
    from meteor_demod_amd import DemodConfig
    return DemodConfig(samplerate=U.REC_SAMPLERATE, bps=16, oqpsk=True)


@functools.lru_cache(maxsize=8)
def recording_cpu(phase_turns: float = 0.0, rs_coded: bool = False):
    """The recording through the CPU demodulator and the host model of the link variant: (soft, first lock symbol, CADUs, frames)."""
    import oracle_py
    from meteor_demod_amd import frames
    _, iq = recording(phase_turns, rs_coded)
    soft, _, events = oracle_py.oracle_demod(recording_cfg(), iq)
    lock = next((s for s, locked in events if locked), None)
    cadu, fr = frames.model_decode(soft, skew=True, differential=True)
    return soft, lock, cadu, fr
