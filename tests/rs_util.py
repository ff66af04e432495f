"""Signals for the transfer-frame layer's tests (test_rs_host.py, test_gpu_rs.py): GF(256) in numpy (independent of the library's
tables), VCDUs with a header, damaged CADUs with a known number of byte errors per codeword, framed streams and one modulated
recording whose frames come from ``rs.model_encode``.  Everything is seeded; what is expensive is made once per process."""
from __future__ import annotations

import functools

import numpy as np

import frames_util as U

N, K, DEPTH, CADU, VCDU, FAILED = 255, 223, 4, 1024, 892, 255
OPTS = [dict(derandomise=d, dual_basis=b) for d in (1, 0) for b in (0, 1)]       # all four combinations


# ------------------------------------------------------------------------------------------------------- the field, in numpy
def _tables():
    exp, log = np.zeros(510, dtype=np.int64), np.zeros(256, dtype=np.int64)
    x = 1
    for i in range(255):
        exp[i] = exp[i + 255] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x187
    return exp, log


EXP, LOG = _tables()


def syndromes(word) -> np.ndarray:
    """The 32 values word(alpha^(11 j)), j = 112 .. 143, of word[0 .. 254] (word[0] the coefficient of x^254)."""
    w = np.asarray(word, dtype=np.int64)
    out = np.zeros(32, dtype=np.int64)
    power = 254 - np.arange(N)
    for k in range(32):
        lroot = (11 * (112 + k)) % 255
        terms = np.where(w == 0, 0, EXP[(LOG[w] + lroot * power) % 255])
        out[k] = np.bitwise_xor.reduce(terms)
    return out


def pn_numpy(count: int = 255) -> np.ndarray:
    """The randomiser from its description: register 0xFF, output bit 7, new bit 0 = b7 ^ b4 ^ b2 ^ b0, MSB first; `count` bytes."""
    reg, out = 0xFF, []
    for _ in range(count):
        byte = 0
        for _ in range(8):
            byte = (byte << 1) | (reg >> 7)
            fb = ((reg >> 7) ^ (reg >> 4) ^ (reg >> 2) ^ reg) & 1
            reg = ((reg << 1) | fb) & 0xFF
        out.append(byte)
    return np.array(out, dtype=np.uint8)


def words(cadu_row, derandomise=1, dual_basis=0) -> np.ndarray:
    """[4, 255]: the four words of one CADU as the decoder sees them (sequence off, Tinv for the dual basis)."""
    from meteor_demod_amd import rs
    body = np.asarray(cadu_row, dtype=np.uint8)[4:].copy()
    if derandomise:
        body ^= np.tile(pn_numpy(), 4)
    if dual_basis:
        body = rs.model_dual()[1][body]
    return body.reshape(N, DEPTH).T.copy()


def plain(cadu_row, derandomise=1, **_) -> np.ndarray:
    """The 892 bytes a decoder leaves when it corrects nothing: the sequence off, nothing else (the dual basis is undone again)."""
    body = np.asarray(cadu_row, dtype=np.uint8)[4:].copy()
    if derandomise:
        body ^= np.tile(pn_numpy(), 4)
    return body[:VCDU]


# ----------------------------------------------------------------------------------------------------------------- frames
def vcdu(rng, vcid: int = 5, counter: int = 0, spacecraft: int = 0x9D) -> np.ndarray:
    """892 bytes: version 1, the given header fields, random data."""
    v = rng.integers(0, 256, VCDU, dtype=np.uint8)
    v[0] = (1 << 6) | (spacecraft >> 2)
    v[1] = ((spacecraft & 3) << 6) | (vcid & 0x3F)
    v[2], v[3], v[4] = (counter >> 16) & 0xFF, (counter >> 8) & 0xFF, counter & 0xFF
    return v


def damage(cadu_row: np.ndarray, c: int, count: int, rng, where=None) -> np.ndarray:
    """`count` byte errors (non-zero differences) into codeword c of one CADU, at distinct positions of `where` (default: all 255).
    Returns the positions."""
    pos = rng.choice(np.arange(N) if where is None else np.asarray(where), count, replace=False)
    for p in pos:
        cadu_row[4 + DEPTH * int(p) + c] ^= np.uint8(rng.integers(1, 256))
    return pos


# the loads a batch cycles through, per codeword: byte errors, or a name
LOADS = [0, 1, 8, 15, 16, 17, 32, "parity", 0, 16, 2, 17]


def mixed_batch(n: int, seed: int, **opts):
    """(sent [n, 892], cadu [n, 1024], loads [n][4]): codeword c of frame f carries LOADS[(5 f + c) % 12] errors ("parity": 9 errors
    in the parity bytes only), so that the four waves of a block and neighbouring blocks take different paths; every seventh frame
    from the fourth on is 1020 random bytes instead ("random" in all four places)."""
    from meteor_demod_amd import rs
    rng = np.random.default_rng(seed)
    sent = np.stack([vcdu(rng, counter=f) for f in range(n)])
    cadu = np.stack([rs.model_encode(v, **opts) for v in sent])
    loads = []
    for f in range(n):
        if f % 7 == 3:
            cadu[f, 4:] = rng.integers(0, 256, N * DEPTH, dtype=np.uint8)
            loads.append(["random"] * DEPTH)
            continue
        row = []
        for c in range(DEPTH):
            load = LOADS[(5 * f + c) % len(LOADS)]
            if load == "parity":
                damage(cadu[f], c, 9, rng, where=np.arange(K, N))
            else:
                damage(cadu[f], c, load, rng)
            row.append(load)
        loads.append(row)
    return sent, cadu, loads


def check_against_what_was_sent(sent, cadu, loads, vcdu_out, info, **opts):
    """The decoding rule on a mixed batch, from what is known about it: up to 16 errors come back as sent with the count; 17 and 32
    errors and random frames are left as received and read 255 (a false correction has probability about 1 / 16!: with fixed seeds
    none occurs)."""
    for f, row in enumerate(loads):
        want_flags = 0
        for c, load in enumerate(row):
            count = 9 if load == "parity" else load
            got = vcdu_out[f, c::DEPTH]
            if load == "random" or count > 16:
                assert info[f, c] == FAILED, (f, c, load, info[f])
                assert np.array_equal(got, plain(cadu[f], **opts)[c::DEPTH]), (f, c, load)
                want_flags = 1
            else:
                assert info[f, c] == count, (f, c, load, info[f])
                assert np.array_equal(got, sent[f, c::DEPTH]), (f, c, load)
        assert int(info[f, 4]) == want_flags and not info[f, 5:].any(), (f, info[f])


# ------------------------------------------------------------------------------------------------------------------ streams
class Stream(U.Stream):
    """frames_util.Stream with frames that are CADUs of ``rs.model_encode``: n_frames VCDUs (counter 0, 1, ...) between `lead` and
    `tail` random bits, encoded without a reset."""

    def __init__(self, seed: int, n_frames: int = 5, lead: int = 777, tail: int = 300, **opts):
        from meteor_demod_amd import rs
        rng = np.random.default_rng(seed)
        self.lead, self.n_frames = lead, n_frames
        self.vcdus = [vcdu(rng, counter=k) for k in range(n_frames)]
        self.frames = [rs.model_encode(v, **opts).tobytes() for v in self.vcdus]
        bits = [rng.integers(0, 2, lead, dtype=np.uint8)]
        bits += [np.unpackbits(np.frombuffer(f, dtype=np.uint8)) for f in self.frames]
        bits += [rng.integers(0, 2, tail, dtype=np.uint8)]
        self.bits = np.concatenate(bits)
        self.sym = U.encode(self.bits).astype(np.float64) * 2 - 1
        self.positions = [lead + U.FRAME * k for k in range(n_frames)]


@functools.lru_cache(maxsize=1)
def stream() -> Stream:
    return Stream(seed=1)


@functools.lru_cache(maxsize=1)
def recording():
    """frames_util.recording() re-made with encoded frames: (Stream, s16 [n, 2])."""
    st = Stream(seed=4242, n_frames=U.REC_FRAMES, lead=3000, tail=600)
    rng = np.random.default_rng(77)
    z = np.zeros(len(st.sym) * U.SPS, dtype=complex)
    z[::U.SPS] = st.sym[:, 0] + 1j * st.sym[:, 1]
    y = np.convolve(z, U._rrc(0.6, U.SPS, 8))
    y = y + np.sqrt(2 / 10 ** 1.3 / 2) * (rng.normal(size=len(y)) + 1j * rng.normal(size=len(y)))
    iq = np.stack([y.real, y.imag], axis=1) * 4000.0
    return st, np.clip(np.rint(iq), -32768, 32767).astype(np.int16)
