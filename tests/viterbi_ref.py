"""An independent maximum-likelihood reference for the frame layer's Viterbi decoder (test_frames_host.py, test_frames_link_host.py,
test_gpu_frames.py, test_gpu_frames_link.py), written from the comment of include/meteor_demod_amd_frames.h and from nothing else:
one pass over a whole array of symbols, 64 states at once in numpy, int64 metrics, every start state at 0, the header's two tie
rules (on equal metrics the predecessor s' >> 1 wins; the traceback starts from the lowest of the best states).  The code itself is
stated once, in frames_util.encode: the branch outputs below are read off that encoder.  Decodings are cached per process, so the
CPU and the GPU tests of one run share them."""
from __future__ import annotations

import functools

import numpy as np

import frames_util as U

FRAME, SUB, HALO = 8192, 1024, 128


@functools.lru_cache(maxsize=1)
def _branches():
    """For each new state s' (the last six input bits, the newest in bit 0): its two predecessors and the +-1 outputs (c1, c2) of
    the two branches, from frames_util.encode on the seven bits of the register."""
    ns = np.arange(64)
    pred = np.stack([ns >> 1, (ns >> 1) | 32])                                # [2, 64]
    out = np.zeros((2, 64, 2), dtype=np.int64)
    for b in range(2):
        for s in range(64):
            reg = ((int(pred[b, s]) << 1) | (s & 1)) & 0x7F                    # bit j: the input j steps ago
            history = [(reg >> j) & 1 for j in range(6, 0, -1)]
            out[b, s] = U.encode(np.array([reg & 1]), np.array(history))[0].astype(np.int64) * 2 - 1
    return pred, out


def ml_decode(sym: np.ndarray):
    """sym int64 [T, 2], already through the hypothesis -> (the T decided bits, the best final metric M*)."""
    sym = np.asarray(sym, dtype=np.int64)
    T = len(sym)
    pred, out = _branches()
    bm0 = sym[:, :1] * out[0, :, 0] + sym[:, 1:] * out[0, :, 1]               # [T, 64]: the branch from s' >> 1
    bm1 = sym[:, :1] * out[1, :, 0] + sym[:, 1:] * out[1, :, 1]               # the branch from (s' >> 1) | 32
    p0, p1 = pred
    pm = np.zeros(64, dtype=np.int64)
    second = np.zeros((T, 64), dtype=bool)
    for t in range(T):
        m0, m1 = pm[p0] + bm0[t], pm[p1] + bm1[t]
        np.greater(m1, m0, out=second[t])                                     # equal: s' >> 1 wins
        pm = np.where(second[t], m1, m0)
    state = int(np.argmax(pm))                                                # the first of the largest: the lowest state
    bits = np.zeros(T, dtype=np.uint8)
    for t in range(T - 1, -1, -1):
        bits[t] = state & 1
        state = (state >> 1) | (int(second[t, state]) << 5)
    return bits, int(pm.max()) if T else 0


def path_metric(bits: np.ndarray, sym: np.ndarray) -> int:
    """The correlation sum I c1 + Q c2 of the re-encoded bits (c as +-1) with sym, maximised over the 64 six-bit histories before
    bit 0: only the first six steps depend on the history."""
    sym = np.asarray(sym, dtype=np.int64)
    bits = np.asarray(bits, dtype=np.uint8)
    tail = int(((U.encode(bits)[6:].astype(np.int64) * 2 - 1) * sym[6:]).sum())
    head = max(int(((U.encode(bits[:6], np.array([(v >> j) & 1 for j in range(6)])).astype(np.int64) * 2 - 1) * sym[:6]).sum()) for v in range(64))
    return head + tail


def nrzm_undo(d: np.ndarray) -> np.ndarray:
    """b[t] = d[t] xor d[t - 1], b[0] = d[0]."""
    d = np.asarray(d, dtype=np.uint8)
    return d ^ np.concatenate([[0], d[:-1]]).astype(np.uint8)


def through_H(soft: np.ndarray, H: int) -> np.ndarray:
    """int64 [m, 2] through the combined hypothesis H = h + 8 s: s = 1 reads (I'[n], Q'[n + 1]), s = 2 (I'[n + 1], Q'[n]); a rail
    value at index m is 0."""
    x = U.through(soft, H & 7).astype(np.int64)
    s = H >> 3
    if s == 1:
        x[:, 1] = np.concatenate([x[1:, 1], [0]])
    elif s == 2:
        x[:, 0] = np.concatenate([x[1:, 0], [0]])
    return x


def windowed_decode(sym: np.ndarray, position: int, differential: bool = False):
    """The header's rule for one frame at `position` of sym (through the hypothesis): eight sub-blocks, each ml_decode on
    [s - 128, s + 1152) clamped to the stream, the middle 1024 bits kept -> (the frame's output bits, the decoder's own bits d).
    With `differential` the output is d[t] xor d[t - 1] within the sub-block's own decoding, 0 before step 0."""
    m = len(sym)
    out, own = [], []
    for k in range(FRAME // SUB):
        s = position + SUB * k
        lo, hi = max(0, s - HALO), min(m, s + SUB + HALO)
        d = ml_decode(sym[lo:hi])[0]
        b = nrzm_undo(d) if differential else d
        out.append(b[s - lo: s - lo + SUB])
        own.append(d[s - lo: s - lo + SUB])
    return np.concatenate(out), np.concatenate(own)


def channel_errors(d: np.ndarray, sym: np.ndarray) -> int:
    """The header's report: hard decisions (value > 0) of a frame's 8192 symbols that differ from the re-encoded bits d, over info
    bits 6..8191, the encoder state taken from the frame's own first six bits."""
    return int(((U.encode(d)[6:] == 1) != (np.asarray(sym)[6:] > 0)).sum())


def bits_of(cadu) -> np.ndarray:
    """CADU bytes ([n, 1024], or one frame's bytes) as one array of bits, MSB first."""
    return np.unpackbits(np.ascontiguousarray(cadu, dtype=np.uint8).reshape(-1))


# ---------------------------------------------------------------------------------- inputs no tracker would hand the decoder
HOSTILE_M = FRAME + 200
HOSTILE_AT = (0, 57, 200, 1, 128, 129, 199, 200)                               # frame positions; the hypotheses cycle over them


def hostile_inputs(hyps=tuple(range(8)), seed: int = 11):
    """[(name, soft int8 [8392, 2], [(position, H), ...])]: all zeros, where every metric ties at every step; symbols drawn from
    {-1, 0, 1}, where most do; the full int8 range with a sixteenth of the symbols forced to -128.  `hyps`: the hypotheses to cycle
    through."""
    rng = np.random.default_rng(seed)
    at = [(p, hyps[k % len(hyps)]) for k, p in enumerate(HOSTILE_AT)]
    zeros = np.zeros((HOSTILE_M, 2), dtype=np.int8)
    ties = rng.integers(-1, 2, (HOSTILE_M, 2)).astype(np.int8)
    full = rng.integers(-128, 128, (HOSTILE_M, 2)).astype(np.int8)
    full[rng.integers(0, HOSTILE_M, HOSTILE_M // 16)] = -128
    return [("zeros", zeros, at), ("ties", ties, at), ("full", full, at)]


def full_scale(st, H: int) -> np.ndarray:
    """The clean stream `st` at full scale, +127 / -128, sent through the inverse of H: a negating hypothesis reads -128 as +128."""
    import link_util as L
    return np.where(L.skew_inverse(st.sym, H) > 0, 127, -128).astype(np.int8)


# ------------------------------------------------------------------------------------------ the streams the ML tests share
ML_SEED = 1                                                                   # frames_util.Stream / link_util.LinkStream seed
ML_RX_SEED = {2.0: 400, 3.0: 500}                                             # receive seed = this + H


@functools.lru_cache(maxsize=None)
def ml_stream(differential: bool = False, lead: int = 0, tail: int = 0):
    """Two frames (m = 16 384 when nothing leads or trails: the frames tile the stream); the link sender's stream without
    `differential` is frames_util.Stream's, bit for bit."""
    import link_util as L
    return L.LinkStream(ML_SEED, n_frames=2, lead=lead, tail=tail, differential=differential)


@functools.lru_cache(maxsize=None)
def ml_case(differential: bool, H: int, esn0_db: float, lead: int = 0, tail: int = 0):
    """(stream, soft int8 [m, 2] sent through the inverse of H, sym through the H the layer reports, d of the full-stream ML
    decoding, M*).  Read-only: the tests share it."""
    import link_util as L
    st = ml_stream(differential, lead, tail)
    soft = st.received(H, esn0_db, seed=ML_RX_SEED[esn0_db] + H)
    sym = through_H(soft, L.canonical(H, differential))
    d, best = ml_decode(sym)
    for a in (soft, sym, d):
        a.setflags(write=False)
    return st, soft, sym, d, best
