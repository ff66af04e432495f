"""Signals for the tests of the 80 k interleaved mode (test_interleave_host.py, test_gpu_interleave.py, test_gpu_interleave_cli.py): a
numpy sender built to the specification in include/meteor_demod_amd_interleave.h - the 36-branch interleaver, the sync word before
every 72 bits, channel symbols sent through the inverse of a combined hypothesis H (link_util.skew_inverse), noise as frames_util
makes it, symbol slips and hypothesis changes - and streams of Reed-Solomon coded frames in front of it.  Everything is seeded; what
is expensive is made once per process."""
from __future__ import annotations

import functools

import numpy as np

import frames_util as U
import link_util as L

BRANCHES, PERIOD, DATA_BITS, WINDOW, SYNC = 36, 40, 72, 2560, 0x27
SYNC_BITS = np.array([(SYNC >> (7 - i)) & 1 for i in range(8)], dtype=np.uint8)


def interleave(u: np.ndarray, M: int, fill: np.ndarray | None = None) -> np.ndarray:
    """v[k] = u[k - 36 M (k mod 36)]; where that index is negative, `fill` (what the sender's registers held; zeros by default)."""
    u = np.asarray(u, dtype=np.uint8)
    k = np.arange(len(u), dtype=np.int64)
    src = k - BRANCHES * M * (k % BRANCHES)
    v = np.zeros(len(u), dtype=np.uint8) if fill is None else np.asarray(fill, dtype=np.uint8)[: len(u)].copy()
    v[src >= 0] = u[src[src >= 0]]
    return v


def channel_symbols(v: np.ndarray) -> np.ndarray:
    """The bits of v (a multiple of 72) with the sync word before every 72: [40 n, 2] of +-1, symbol i = (c[2 i], c[2 i + 1])."""
    rows = np.asarray(v, dtype=np.uint8).reshape(-1, DATA_BITS)
    c = np.concatenate([np.tile(SYNC_BITS, (len(rows), 1)), rows], axis=1).reshape(-1)
    return c.reshape(-1, 2).astype(np.float64) * 2 - 1


class Sender:
    """u (0 / 1, cut to whole periods of 72 bits) through the interleaver with branch delay M, behind `lead` random symbols (< 40:
    the phase of the first sync word).  `events` is a list of (symbol index in the sent stream, kind, argument): ("delete", None)
    drops that symbol, ("insert", None) puts a random symbol before it, ("hyp", H) changes the hypothesis from that symbol on."""

    def __init__(self, u: np.ndarray, M: int, lead: int = 0, seed: int = 0, events=(), tail: int = 1):
        rng = np.random.default_rng(seed)
        u = np.asarray(u, dtype=np.uint8)
        self.u = u[: len(u) // DATA_BITS * DATA_BITS]
        self.M, self.lead, self.events = M, lead, sorted(events)
        self.periods = len(self.u) // DATA_BITS
        v = interleave(self.u, M, fill=rng.integers(0, 2, len(self.u), dtype=np.uint8))
        # (`tail` random symbols behind the last period: under a skewed H the last period's late rail is still inside the stream)
        self.sym = np.concatenate([rng.integers(0, 2, (lead, 2)) * 2.0 - 1, channel_symbols(v), rng.integers(0, 2, (tail, 2)) * 2.0 - 1])

    def received(self, H: int, esn0_db: float | None, seed: int) -> np.ndarray:
        """int8 [m, 2] sent through the inverse of H (and of what the events change it to): amplitude 48, Gaussian noise (none for
        esn0_db None), rounded and clipped; the events applied."""
        rng = np.random.default_rng(seed)
        pieces, at, h = [], 0, H
        for e, kind, arg in self.events:
            pieces.append(L.skew_inverse(self.sym, h)[at:e])
            at = e
            if kind == "hyp":
                h = arg
            elif kind == "delete":
                at = e + 1
            elif kind == "insert":
                pieces.append(rng.integers(0, 2, (1, 2)) * 2.0 - 1)
        pieces.append(L.skew_inverse(self.sym, h)[at:])
        x = np.concatenate(pieces)
        if esn0_db is None:
            return U.quantise(U.AMP * x)
        return U.quantise(U.AMP * x + U.sigma_of(esn0_db) * rng.normal(size=x.shape))

    def source_symbol(self, k: np.ndarray) -> np.ndarray:
        """The index, in the sent stream, of the channel symbol that carries output bit k (u[k])."""
        kp = np.asarray(k, dtype=np.int64) + BRANCHES * self.M * (np.asarray(k, dtype=np.int64) % BRANCHES)
        return self.lead + PERIOD * (kp // DATA_BITS) + 4 + (kp % DATA_BITS) // 2

    def far_from_events(self, k: np.ndarray, distance: int = 2 * WINDOW) -> np.ndarray:
        x = self.source_symbol(k)
        far = np.ones(len(x), dtype=bool)
        for e, _, _ in self.events:
            far &= np.abs(x - e) >= distance
        return far


def random_sender(seed: int, periods: int, M: int, lead: int = 0, events=()) -> Sender:
    return Sender(np.random.default_rng(seed).integers(0, 2, DATA_BITS * periods, dtype=np.uint8), M, lead, seed + 1, events)


# the slip / rotation stream of the specification: 3000 periods; one symbol deleted, H 9 -> 20, one symbol inserted, each late in a
# window (the window's candidate is still the old one) and at least 11 windows apart.  From hypothesis 9.
SLIP_LEAD, SLIP_H = 17, (9, 20)
SLIP_EVENTS = ((11 * WINDOW + 2000, "delete", None), (22 * WINDOW + 2000, "hyp", 20), (34 * WINDOW + 2000, "insert", None))
SLIP_PERIODS = (0, 768, 1472, 2240)                                             # N0 of the four segments


@functools.lru_cache(maxsize=4)
def slip_sender(M: int = 8) -> Sender:
    return random_sender(31, 3000, M, SLIP_LEAD, SLIP_EVENTS)


def check_bits(sender: Sender, out: np.ndarray, n_periods: int):
    """The gather's output against the sender: every bit with N < P whose source is at least two windows from every event has the
    sender's hard decision, every bit with N >= P is exactly 0.  Returns (bits compared, bits excluded near an event, bits)."""
    flat = np.asarray(out).reshape(-1)
    n = min(len(flat), len(sender.u))
    k = np.arange(n, dtype=np.int64)
    N = (k + BRANCHES * sender.M * (k % BRANCHES)) // DATA_BITS
    have = N < n_periods
    assert (flat[:n][~have] == 0).all()
    far = sender.far_from_events(k) & have
    wrong = np.flatnonzero((flat[:n][far] > 0) != (sender.u[:n][far] > 0))
    assert wrong.size == 0, (wrong.size, wrong[:10])
    return int(far.sum()), int((have & ~far).sum()), n


# ---------------------------------------------------------------------------------------------------------- framed streams
class FramedSender(Sender):
    """n_frames Reed-Solomon coded, randomised transfer frames (rs_util / rs.model_encode) between `lead_bits` and `tail_bits`
    random bits, NRZ-M coded with `differential`, through the K = 7 encoder (u[2 n] = c1, u[2 n + 1] = c2) and the interleaver."""

    def __init__(self, seed: int, M: int, n_frames: int = 4, lead_bits: int = 777, tail_bits: int = 300, differential: bool = False, lead: int = 0):
        import rs_util
        from meteor_demod_amd import rs
        rng = np.random.default_rng(seed)
        self.vcdus = [rs_util.vcdu(rng, counter=k) for k in range(n_frames)]
        self.frames = [rs.model_encode(v).tobytes() for v in self.vcdus]
        bits = [rng.integers(0, 2, lead_bits, dtype=np.uint8)]
        bits += [np.unpackbits(np.frombuffer(f, dtype=np.uint8)) for f in self.frames]
        bits += [rng.integers(0, 2, tail_bits, dtype=np.uint8)]
        bits = np.concatenate(bits)
        coded = L.nrzm(bits) if differential else bits
        super().__init__(U.encode(coded).reshape(-1), M, lead, seed + 1)
        self.positions = [lead_bits + U.FRAME * k for k in range(n_frames)]


def tail_bits_for(M: int, n_frames: int, lead_bits: int) -> int:
    """Info bits behind the frames so that every coded bit of the frames (and of 200 symbols after them) has left the interleaver
    before the stream ends: frames' end + 35 x 36 M bits <= stream length."""
    return (35 * BRANCHES * M + 400) // 2 + DATA_BITS


# ---------------------------------------------------------------------------------------------------------- the recording
REC_M, REC_NOISE_SEED = 8, 79


@functools.lru_cache(maxsize=2)
def recording(differential: bool = False):
    """(FramedSender, s16 [n, 2]): 9 RS-coded frames, interleaved with M = 8, as OQPSK - the Q rail two samples (half a symbol)
    late - RRC 0.6, 4 samples per symbol, carrier at 0 Hz, Es/N0 about 13 dB: built like link_util.recording."""
    st = FramedSender(seed=4244, M=REC_M, n_frames=U.REC_FRAMES, lead_bits=3000, tail_bits=tail_bits_for(REC_M, U.REC_FRAMES, 3000) + 4600,
                      differential=differential)
    rng = np.random.default_rng(REC_NOISE_SEED)
    n = len(st.sym) * U.SPS
    zi, zq = np.zeros(n + U.SPS // 2), np.zeros(n + U.SPS // 2)
    zi[: n: U.SPS] = st.sym[:, 0]
    zq[U.SPS // 2: n + U.SPS // 2: U.SPS] = st.sym[:, 1]
    pulse = U._rrc(0.6, U.SPS, 8)
    y = np.convolve(zi, pulse) + 1j * np.convolve(zq, pulse)                   # unit-energy pulse: Es = 2
    y = y + np.sqrt(2 / 10 ** 1.3 / 2) * (rng.normal(size=len(y)) + 1j * rng.normal(size=len(y)))
    iq = np.stack([y.real, y.imag], axis=1) * 4000.0
    return st, np.clip(np.rint(iq), -32768, 32767).astype(np.int16)
