"""Helpers of the tap-exact front-end tests (no GPU): the geometries and the branch of fe_plan each reaches, impulse trains whose
responses are the taps themselves, the call cuts, float64 and float32 models of mixer and filter.

Why impulses: the kernel sums y[m] = sum_k h[k] z[m D - k] with one FMA per tap on a zero accumulator.  Where z is zero except
one sample, every product but one is a zero, so the output is np.float32(h[k]) * np.float32(a) - one rounding - whatever the
order of the sum, the tile, the number of threads that share an output or the call the sample arrived in.  A lost, doubled or
shifted tap is then a different float, not a small error."""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np

from conftest import ROOT

SYMRATE = 72000
FE_SOURCE = ROOT / "meteor_demod_amd" / "csrc" / "frontend.hip"

# (D, taps_per_phase) and what fe_plan makes of it: ("R", outputs per thread) or ("G", threads per output)
GEOMETRIES = [
    (1, 16, ("R", 4)),
    (3, 8, ("R", 4)),
    (5, 16, ("R", 4)),
    (8, 16, ("R", 2)),
    (13, 16, ("R", 1)),
    (24, 32, ("G", 2)),
    (65, 16, ("G", 4)),
    (128, 16, ("G", 8)),
    (128, 32, ("G", 16)),
    (100, 32, ("G", 16)),
]
CASES = [(d, tpp) for d, tpp, _ in GEOMETRIES]
ALL_FORMATS = [(5, 16), (13, 16), (24, 32), (100, 32)]       # u8, s16 and f32 here; f32 alone elsewhere


def case_id(case) -> str:
    return f"D{case[0]}x{case[1]}"


def n_taps(d: int, tpp: int) -> int:
    return 1 if d == 1 else tpp * d + 1


def source_constants() -> dict:
    """FE_BLOCK and FE_SPAN_MAX as csrc/frontend.hip defines them."""
    text = FE_SOURCE.read_text()
    return {name: int(re.search(rf"^#define\s+{name}\s+(\d+)", text, re.M).group(1)) for name in ("FE_BLOCK", "FE_SPAN_MAX")}


def plan(d: int, tpp: int, block: int | None = None, span_max: int | None = None) -> dict:
    """fe_plan's arithmetic restated: T outputs per tile, R outputs per thread (G == 1) or G threads per output, and the phase
    range [lo, hi) of each of the G threads."""
    if block is None or span_max is None:
        c = source_constants()
        block, span_max = c["FE_BLOCK"], c["FE_SPAN_MAX"]
    L = n_taps(d, tpp)
    G = R = T = 0
    for r in (4, 2, 1):
        if not G and (block * r - 1) * d + L <= span_max:
            G, R, T = 1, r, block * r
    g = 2
    while not G and g <= block:
        if g <= d and (block // g - 1) * d + L <= span_max:
            G, R, T = g, 1, block // g
        g *= 2
    assert G, (d, tpp)
    per = -(-d // G)
    ranges = [(i * per, max(i * per, min(i * per + per, d))) for i in range(G)]
    return dict(D=d, L=L, H=L - 1, G=G, R=R, T=T, span=(T - 1) * d + L, per=per, ranges=ranges)


def branch(d: int, tpp: int):
    p = plan(d, tpp)
    return ("R", p["R"]) if p["G"] == 1 else ("G", p["G"])


def configs(d: int, tpp: int, bps: int, offset: float = 0.0, fs: int | None = None):
    """(DemodConfig, FrontEndConfig) at the input rate 250 kS/s x D."""
    from meteor_demod_amd import DemodConfig, FrontEndConfig
    return DemodConfig(samplerate=fs or 250000 * d, symrate=SYMRATE, bps=bps), FrontEndConfig(offset, d, tpp)


def taps(d: int, tpp: int, bps: int = 32) -> np.ndarray:
    from meteor_demod_amd import design_taps
    h, _ = design_taps(*configs(d, tpp, bps))
    assert len(h) == n_taps(d, tpp) and h.dtype == np.float32
    return h


# ------------------------------------------------------------------------------------------------------------ impulse trains
_NP = {8: np.uint8, 16: np.int16, 32: np.float32}


@dataclass
class Train:
    d: int
    L: int
    bps: int
    x: np.ndarray            # [n, 2] in the input's format
    at: np.ndarray           # impulse positions, ascending
    val: np.ndarray          # [len(at), 2] float32: the converted values (u8: minus 128)

    @property
    def n(self) -> int:
        return len(self.x)


def impulse_train(d: int, L: int, bps: int, seed: int, first: int = 0) -> Train:
    """Zero (u8: 128) except D impulses at first + i S, S = 1 mod D and S > L + D: one impulse for every residue mod D, no two
    responses overlapping; behind the last response a tail that is no multiple of D."""
    rng = np.random.default_rng(seed)
    S = d * -(-(L + d) // d) + 1
    at = first + S * np.arange(d, dtype=np.int64)
    assert sorted(at % d) == list(range(d)) and S >= L + d
    n = int(at[-1]) + L + d + 3
    n += 1 if d > 1 and n % d == 0 else 0
    if bps == 32:
        raw = rng.uniform(-4.0, 4.0, size=(d, 2)).astype(np.float32)
        raw[raw == 0.0] = 1.0
    elif bps == 16:
        raw = rng.integers(-32768, 32768, size=(d, 2)).astype(np.int16)
        raw[raw == 0] = 3
        special = np.array([1, -1, 32767, -32768, -1, 32767, -32768, 1], dtype=np.int16)
        raw.reshape(-1)[: min(len(special), 2 * d)] = special[: 2 * d]
    else:
        raw = rng.integers(0, 256, size=(d, 2)).astype(np.uint8)
        raw[raw == 128] = 131
        special = np.array([0, 255, 255, 0, 127, 129], dtype=np.uint8)
        raw.reshape(-1)[: min(len(special), 2 * d)] = special[: 2 * d]
    x = np.full((n, 2), 128 if bps == 8 else 0, dtype=_NP[bps])
    x[at] = raw
    val = raw.astype(np.float32) - np.float32(128 if bps == 8 else 0)
    assert np.all(val != 0)
    return Train(d, L, bps, x, at, val)


def reach(train: Train, n: int | None = None):
    """For every impulse the outputs it reaches among the first ceil(n / D) and the tap that reaches each: (i, m, k) arrays."""
    n = train.n if n is None else n
    n_out = -(-n // train.d)
    ii, mm, kk = [], [], []
    for i, a in enumerate(train.at):
        if a >= n:
            continue
        m = np.arange(-(-int(a) // train.d), min((int(a) + train.L - 1) // train.d + 1, n_out), dtype=np.int64)
        ii.append(np.full(len(m), i))
        mm.append(m)
        kk.append(m * train.d - int(a))
    if not ii:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    return np.concatenate(ii), np.concatenate(mm), np.concatenate(kk)


def taps_hit(train: Train) -> set:
    return set(reach(train)[2].tolist())


def expected(train: Train, h: np.ndarray, n: int | None = None) -> np.ndarray:
    """The baseband of the first n samples, float32 [ceil(n / D), 2]: np.float32(h[k]) * np.float32(a) where an impulse reaches,
    0 elsewhere."""
    n = train.n if n is None else n
    out = np.zeros((-(-n // train.d), 2), dtype=np.float32)
    i, m, k = reach(train, n)
    assert len(set(m.tolist())) == len(m), "two responses overlap"
    out[m] = h.astype(np.float32)[k, None] * train.val[i]
    return out


# ---------------------------------------------------------------------------------------------------------------------- cuts
def cut_sizes(d: int, H: int) -> list:
    return [s for s in (1, d - 1, d, d + 1, 0, H - 1, H, H + 1, 3 * H + 7, 65521) if s >= 0]


def cuts(n: int, d: int, H: int, start: int = 0) -> list:
    """Call sizes that sum to n, cycling through cut_sizes from entry `start`."""
    sizes = cut_sizes(d, H)
    out, at, i = [], 0, start
    while at < n:
        k = min(sizes[i % len(sizes)], n - at)
        out.append(k)
        at += k
        i += 1
    assert sum(out) == n
    return out


def cut_properties(calls, at, L: int):
    """(a call of 1 .. H - 1 samples begins while the history holds an impulse, so that the new history is built from the old one;
    a boundary falls inside a response)."""
    H = L - 1
    bounds = np.cumsum(calls)[:-1]
    starts = np.concatenate([[0], bounds])
    short = any(0 < k < H and np.any((s > at) & (s < at + L)) for k, s in zip(calls, starts))
    inside = any(np.any((bounds > a) & (bounds < a + L)) for a in at)
    return bool(short), bool(inside)


def cuts_for(train: Train) -> list:
    """The cut of train.n whose cycle start makes a response straddle a boundary and a short call follow a response (asserted
    where there is a history at all).  At most a couple of hundred calls."""
    H = train.L - 1
    n_sizes = len(cut_sizes(train.d, H))
    for start in range(n_sizes):
        c = cuts(train.n, train.d, H, start)
        if H < 2 or all(cut_properties(c, train.at, train.L)):
            assert len(c) <= 300, len(c)
            return c
    raise AssertionError(f"no cycle start cuts a response of D={train.d}, L={train.L}")


# -------------------------------------------------------------------------------------------------------------------- models
def to_complex(x: np.ndarray, bps: int, dtype=np.float64) -> np.ndarray:
    xc = x.astype(dtype) - dtype(128 if bps == 8 else 0)
    return xc[:, 0] + 1j * xc[:, 1]


def phase_words(step: int, n: int, n0: int = 0) -> np.ndarray:
    """p(n) = n step mod 2^32 for the absolute indices n0 .. n0 + n - 1."""
    idx = np.arange(n0, n0 + n, dtype=np.uint64)
    return (idx * np.uint64(step)) & np.uint64(0xFFFFFFFF)


def mix64(z: np.ndarray, step: int, n0: int = 0) -> np.ndarray:
    """float64: z e^{j 2 pi p(n) / 2^32}, the full 32 bits of the phase, n absolute from n0."""
    if not step:
        return z.astype(np.complex128)
    return z * np.exp(2j * np.pi * phase_words(step, len(z), n0).astype(np.float64) / 2.0 ** 32)


def table_indices(p: np.ndarray):
    """The entries of the two 1024-entry tables that fe_mix reads for the phase words p."""
    p20 = ((p + np.uint64(0x800)) >> np.uint64(12)) & np.uint64(0xFFFFF)
    return (p20 >> np.uint64(10)).astype(np.int64), (p20 & np.uint64(1023)).astype(np.int64)


def mix32(z: np.ndarray, step: int, n0: int = 0) -> np.ndarray:
    """fe_mix restated in float32 (complex64 in and out): the phase rounded to 20 bits, the two tables computed in double and
    rounded once, every product and sum rounded on its own."""
    z = z.astype(np.complex64)
    if not step:
        return z
    hi, lo = table_indices(phase_words(step, len(z), n0))
    i = np.arange(1024, dtype=np.float64)
    f = np.float32
    ax, ay = np.cos(2 * np.pi * i / 1024.0).astype(f)[hi], np.sin(2 * np.pi * i / 1024.0).astype(f)[hi]
    bx, by = np.cos(2 * np.pi * i / 1048576.0).astype(f)[lo], np.sin(2 * np.pi * i / 1048576.0).astype(f)[lo]
    c, s = ax * bx - ay * by, ax * by + ay * bx
    xr, xi = z.real.astype(f), z.imag.astype(f)
    return ((xr * c - xi * s) + 1j * (xr * s + xi * c)).astype(np.complex64)


def filter_model(z: np.ndarray, h: np.ndarray, d: int, dtype) -> np.ndarray:
    """y[m] = sum_k h[k] z[m D - k] for m = 0 .. ceil(len(z) / D) - 1, zero history, in the kernel's order: phases r ascending,
    columns q ascending, z[m D - H + q D + r] at its tap h[H - q D - r] (the kernel reads h[q D + r] there: the design is symmetric
    bit for bit), one multiply and one add per tap, vectorised over m.  `dtype` complex128 is the reference, complex64 the float32
    yardstick."""
    real = np.float64 if dtype == np.complex128 else np.float32
    L, H = len(h), len(h) - 1
    n_out = -(-len(z) // d)
    zp = np.zeros(H + n_out * d + 1, dtype=dtype)
    zp[H: H + len(z)] = z.astype(dtype)
    hh = h.astype(real)
    acc = np.zeros(n_out, dtype=dtype)
    base = np.arange(n_out, dtype=np.int64) * d
    for r in range(d):
        for k in range(r, L, d):
            acc = acc + hh[H - k] * zp[base + k]
    return acc


def dense_input(bps: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if bps == 8:
        return rng.integers(0, 256, size=(n, 2)).astype(np.uint8)
    if bps == 16:
        return np.clip(rng.normal(0, 3000, size=(n, 2)), -32768, 32767).astype(np.int16)
    return rng.normal(0, 0.3, size=(n, 2)).astype(np.float32)
