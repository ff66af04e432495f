"""GPU tests of fe_filter / fe_advance (csrc/frontend.hip) that need no tolerance where the arithmetic allows none: impulse
responses are the taps, float for float, at every branch of fe_plan and across call boundaries; the mixer against float64 with a
bar derived from its arithmetic; dense input against float64 with a bar measured on a float32 CPU evaluation of the same sum;
batch, capacity and reset at a shared-output geometry.  The helpers are in tests/frontend_util.py; every test prints the figures
it asserts on."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import frontend_util as U

pytestmark = pytest.mark.gpu


def _pairs(y: np.ndarray) -> np.ndarray:
    return y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)


def _run(cfg, fe, xd, calls):
    """One FrontEnd over xd [n, 2] cut into `calls`: the outputs of all calls, float32 [ceil(n / D), 2].  Every call's count is
    ceil((n_abs + k) / D) - ceil(n_abs / D)."""
    from meteor_demod_amd import FrontEnd
    d = fe.decimation
    parts, at = [], 0
    with FrontEnd(cfg, fe, 1) as f:
        for k in calls:
            bb, c = f.baseband(xd[at: at + k].reshape(1, k, 2))
            assert int(c[0]) == -(-(at + k) // d) - -(-at // d), (at, k, int(c[0]))
            parts.append(bb[0, : int(c[0])].cpu().numpy())
            at += k
    assert at == xd.shape[0]
    return np.concatenate(parts)


def _device(x: np.ndarray, gpu_device):
    import torch
    return torch.from_numpy(x).to(f"cuda:{gpu_device}")


# ---------------------------------------------------------------------------------------------------- A1: impulses, no mixer
_A1 = [(case, 32) for case in U.CASES] + [(case, bps) for case in U.ALL_FORMATS for bps in (16, 8)]


@pytest.mark.parametrize("case,bps", _A1, ids=[f"{U.case_id(c)}-{b}" for c, b in _A1])
def test_impulse_responses_are_the_taps_exactly(case, bps, gpu_device):
    """D impulses, one per residue mod D, no two responses overlapping: every output is np.float32(h[k]) * np.float32(a) where an
    impulse reaches it and 0.0 elsewhere (np.array_equal), ceil(N / D) outputs, every tap 0 .. L-1 hit - in one call and on one
    FrontEnd cut into calls of 1, D - 1, D, D + 1, 0, H - 1, H, H + 1, 3 H + 7 and 65521 samples."""
    d, tpp = case
    cfg, fe = U.configs(d, tpp, bps)
    h = U.taps(d, tpp, bps)
    tr = U.impulse_train(d, len(h), bps, seed=100 * d + tpp + bps)
    assert U.taps_hit(tr) == set(range(len(h)))
    want = U.expected(tr, h)
    xd = _device(tr.x, gpu_device)
    calls = U.cuts_for(tr)
    for name, cs in (("one call", [tr.n]), (f"{len(calls)} calls", calls)):
        got = _run(cfg, fe, xd, cs)
        assert got.dtype == np.float32 and got.shape == (-(-tr.n // d), 2) == want.shape
        wrong = int(np.count_nonzero((got != want).any(axis=1)))
        print(f"impulses D={d} tpp={tpp} bps={bps} {U.branch(d, tpp)} {name}: {len(got)} outputs, {np.count_nonzero(want[:, 0])} "
              f"reached, {wrong} differ")
        assert np.array_equal(got, want), (name, np.flatnonzero((got != want).any(axis=1))[:8])


# ------------------------------------------------------------------------------------------------------- A2: the mixer alone
@pytest.mark.parametrize("bps", [16, 32])
def test_mixer_alone_against_float64(bps, gpu_device):
    """D = 1 (L = 1, h = [1]: the baseband is the mixed sample), fs = 1 MS/s, offset 123 456.7 Hz, 2^21 samples of (12345, -7001)
    in cut calls: every output within 4e-6 |x| of x e^{j 2 pi p(n) / 2^32} at the absolute n.  The bar: the phase rounded to 20
    bits (2 pi 2^-21 = 3.0e-6 rad at most) plus 16 float32 roundings (16 x 2^-24 = 9.5e-7); the float32 restatement of fe_mix
    gives 3.11e-6 on the CPU, and the kernel 3.112e-6 on an MI355X in both formats; a one-sample slip of the index is 0.78 rad.
    All 1024 entries of both tables occur."""
    from meteor_demod_amd.frontend import phase_step
    fs, off, n = 1000000, 123456.7, 1 << 21
    cfg, fe = U.configs(1, 16, bps, offset=off, fs=fs)
    step = phase_step(off, fs)
    assert U.taps(1, 16).tolist() == [1.0]
    hi, lo = U.table_indices(U.phase_words(step, n))
    assert set(hi.tolist()) == set(range(1024)) and set(lo.tolist()) == set(range(1024))
    x = np.empty((n, 2), dtype={16: np.int16, 32: np.float32}[bps])
    x[:, 0], x[:, 1] = 12345, -7001
    z = U.to_complex(x, bps)
    calls = U.cuts(n, 1, 0)
    assert len(calls) <= 300 and {0, 1, 2, 7, 65521} <= set(calls)
    got = _pairs(_run(cfg, fe, _device(x, gpu_device), calls))
    want = U.mix64(z, step)
    err = float(np.abs(got - want).max() / abs(z[0]))
    ref = float(np.abs(U.mix32(z, step).astype(np.complex128) - want).max() / abs(z[0]))
    print(f"mixer bps={bps}: {len(calls)} calls, max|err|/|x| = {err:.3e} (float32 restatement on the CPU: {ref:.3e}); "
          f"one sample off would be {2 * np.pi * min(step, 2 ** 32 - step) / 2.0 ** 32:.2f} rad")
    assert err <= 4e-6, err


# ------------------------------------------------------------------------------------- A3: mixer and filter across calls
@pytest.mark.parametrize("case", [(8, 16), (24, 32), (100, 32)], ids=U.case_id)
def test_mixed_impulses_across_calls(case, gpu_device):
    """The impulse trains at offset -0.37 fs, s16: each output within 4.2e-6 |h[k]| |x| of h[k] x e^{j theta(n_i)} (the mixer's
    4e-6 and the product's rounding), exactly 0 where no impulse reaches; in one call and in cut calls, which give the one-call
    bytes."""
    from meteor_demod_amd.frontend import phase_step
    d, tpp = case
    fs = 250000 * d
    cfg, fe = U.configs(d, tpp, 16, offset=-0.37 * fs)
    step = phase_step(-0.37 * fs, fs)
    h = U.taps(d, tpp, 16)
    tr = U.impulse_train(d, len(h), 16, seed=7 * d + tpp)
    i, m, k = U.reach(tr)
    xi = tr.val[:, 0].astype(np.float64) + 1j * tr.val[:, 1].astype(np.float64)
    rot = np.exp(2j * np.pi * U.phase_words(step, int(tr.at[-1]) + 1)[tr.at].astype(np.float64) / 2.0 ** 32)
    want = np.zeros(-(-tr.n // d), dtype=np.complex128)
    want[m] = h.astype(np.float64)[k] * (xi * rot)[i]
    bar = np.zeros(len(want))
    bar[m] = 4.2e-6 * np.abs(h.astype(np.float64)[k]) * np.abs(xi)[i]
    xd = _device(tr.x, gpu_device)
    calls = U.cuts_for(tr)
    one = _run(cfg, fe, xd, [tr.n])
    many = _run(cfg, fe, xd, calls)
    for name, got in (("one call", one), (f"{len(calls)} calls", many)):
        err = np.abs(_pairs(got) - want)
        worst = float((err[m] / (bar[m] / 4.2e-6)).max())
        print(f"mixed impulses D={d} tpp={tpp} {name}: max|err| / (|h[k]| |x|) = {worst:.3e}, "
              f"{int(np.count_nonzero(err[bar == 0]))} nonzero where nothing reaches")
        assert np.all(err <= bar), (name, worst)
    assert one.tobytes() == many.tobytes()


# ------------------------------------------------------------------------------------------------------- A4: dense input
@pytest.mark.parametrize("bps", [16, 32])
@pytest.mark.parametrize("mixed", [False, True], ids=["centre", "offset"])
@pytest.mark.parametrize("case", [(65, 16), (128, 32), (100, 32)], ids=U.case_id)
def test_dense_input_against_float64_with_a_measured_bar(case, mixed, bps, gpu_device):
    """Seeded noise through cut calls against the float64 model (the mixer at the absolute index of each call).  The bar is 4
    times the largest error of a float32 CPU evaluation of the same sum in the kernel's order (one multiply and one add per tap,
    neither fused nor split over G threads: both change the error by less than a factor of 2).
    Measured on an MI355X, max|err| kernel / float32 yardstick, in units of the input's RMS (s16, f32):
      (65, 16)   offset 0: 1.24e-7 / 4.46e-7, 1.33e-7 / 5.10e-7;   -0.37 fs: 5.38e-7 / 5.69e-7, 6.13e-7 / 7.49e-7
      (128, 32)  offset 0: 7.77e-8 / 4.29e-7, 7.04e-8 / 3.90e-7;   -0.37 fs: 4.22e-7 / 4.70e-7, 4.18e-7 / 5.92e-7
      (100, 32)  offset 0: 1.17e-7 / 6.11e-7, 7.58e-8 / 4.49e-7;   -0.37 fs: 4.94e-7 / 6.40e-7, 4.95e-7 / 5.88e-7
    The kernel is at 0.17 .. 0.28 of the yardstick without the mixer (the FMA and the G partial sums round less often) and at
    0.71 .. 0.94 with it, where the 20-bit phase, which both share, is most of the error."""
    from meteor_demod_amd.frontend import phase_step
    d, tpp = case
    fs = 250000 * d
    off = -0.37 * fs if mixed else 0.0
    cfg, fe = U.configs(d, tpp, bps, offset=off)
    step = phase_step(off, fs)
    h = U.taps(d, tpp, bps)
    H = len(h) - 1
    n = 2 * sum(U.cut_sizes(d, H)) + 12345
    x = U.dense_input(bps, n, seed=d * 10 + bps)
    z = U.to_complex(x, bps)
    rms = float(np.sqrt((np.abs(z) ** 2).mean()))
    calls = U.cuts(n, d, H)
    got = _pairs(_run(cfg, fe, _device(x, gpu_device), calls))
    at = np.concatenate([[0], np.cumsum(calls)])
    z64 = np.concatenate([U.mix64(z[a: a + k], step, n0=int(a)) for a, k in zip(at, calls)])
    want = U.filter_model(z64, h, d, np.complex128)
    yard = U.filter_model(U.mix32(z, step), h, d, np.complex64).astype(np.complex128)
    assert len(got) == len(want) == -(-n // d)
    e_k, e_y = float(np.abs(got - want).max()), float(np.abs(yard - want).max())
    print(f"dense D={d} tpp={tpp} bps={bps} offset={off:.0f}: {len(calls)} calls, {len(got)} outputs, max|err|/rms kernel {e_k / rms:.3e}, "
          f"float32 yardstick {e_y / rms:.3e}, ratio {e_k / e_y:.2f}")
    assert e_k <= 4.0 * e_y, (e_k / rms, e_y / rms)


# --------------------------------------------------------------------------------------- A5: batch, capacity and reset
def test_batch_capacity_and_reset_at_a_shared_output_geometry(gpu_device):
    """D = 24, 32 taps per phase (G = 2), five streams of ragged counts (one 0), each its own impulse train at its own place in one
    flat buffer: every row exact.  Then mdemod_fe_baseband_device with bb_cap half the outputs of the largest count on rows full
    of a canary: n_out = min(produced, bb_cap), the kept outputs exact, nothing past bb_cap written, and the following
    full-capacity call gives the outputs of an uncut run at those indices.  After reset() the first call is a fresh front end's."""
    import torch
    from meteor_demod_amd import FrontEnd, frontend
    d, tpp, ns = 24, 32, 5
    cfg, fe = U.configs(d, tpp, 16)
    h = U.taps(d, tpp, 16)
    L = len(h)
    trains = [U.impulse_train(d, L, 16, seed=50 + s, first=(0, 5, 11, 17, 23)[s]) for s in range(ns)]
    counts = [trains[0].n, trains[1].n - 1001, 0, int(trains[3].at[7]) + 300, trains[4].n - 13]
    first = [int(trains[0].at[11]) + 100, int(trains[1].at[3]) + 1, 0, counts[3], int(trains[4].at[20]) + L - 2]
    rest = [c - a for c, a in zip(counts, first)]
    assert all(0 <= a <= c for a, c in zip(first, counts)) and rest[3] == 0 and 0 < rest[0] and counts[2] == 0
    gap = 37
    offs, pieces, at = [], [], 0
    for s in range(ns):
        pieces.append(np.full((gap, 2), 9999, dtype=np.int16))           # (what no stream may read)
        offs.append(at + gap)
        pieces.append(trains[s].x[: counts[s]])
        at += gap + counts[s]
    pieces.append(np.full((gap, 2), 9999, dtype=np.int16))
    flat = _device(np.concatenate(pieces), gpu_device)
    dev = flat.device

    def i64(v):
        return torch.tensor(v, dtype=torch.int64, device=dev)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)

    def outs(c):
        return -(-c // d)

    def check_rows(tag, bb, n_out, want_rows):
        for s in range(ns):
            assert int(n_out[s]) == len(want_rows[s]), (tag, s, int(n_out[s]), len(want_rows[s]))
            row = bb[s, : int(n_out[s])]
            print(f"{tag} stream {s}: {len(row)} outputs, {int(np.count_nonzero((row != want_rows[s]).any(axis=1)))} differ")
            assert np.array_equal(row, want_rows[s]), (tag, s)

    whole = [U.expected(trains[s], h, counts[s]) for s in range(ns)]
    with FrontEnd(cfg, fe, ns) as f:
        bb, n_out = f.baseband_ragged(flat, i64(offs), i32(counts), max(counts))
        torch.cuda.synchronize()
        check_rows("ragged", bb.cpu().numpy(), n_out.cpu().numpy(), whole)

        # the same streams in two calls, the first with half the room
        f.reset()
        stride = outs(max(counts))
        cap = outs(max(first)) // 2
        assert any(outs(a) > cap for a in first) and any(0 < outs(a) < cap for a in first)
        canary = np.float32(-7777.25)
        rows = torch.full((ns, stride, 2), float(canary), dtype=torch.float32, device=dev)
        got_n = torch.full((ns,), -1, dtype=torch.int32, device=dev)
        o1, c1 = i64(offs), i32(first)
        frontend.check(frontend.lib().mdemod_fe_baseband_device(f._h, C.c_void_p(flat.data_ptr()), C.c_void_p(o1.data_ptr()),
                                                                  C.c_void_p(c1.data_ptr()), C.c_void_p(rows.data_ptr()), stride, cap,
                                                                  C.c_void_p(got_n.data_ptr()), f._stream()), "mdemod_fe_baseband_device")
        torch.cuda.synchronize()
        rows_h, got_h = rows.cpu().numpy(), got_n.cpu().numpy()
        print(f"capped: bb_cap {cap} of row pitch {stride}, produced {[outs(a) for a in first]}, n_out {got_h.tolist()}")
        assert got_h.tolist() == [min(outs(a), cap) for a in first]
        check_rows("capped", rows_h, got_h, [whole[s][: min(outs(first[s]), cap)] for s in range(ns)])
        assert np.all(rows_h[:, cap:] == canary), "written past bb_cap"
        bb, n_out = f.baseband_ragged(flat, i64([o + a for o, a in zip(offs, first)]), i32(rest), max(max(rest), 1))
        torch.cuda.synchronize()
        check_rows("after the capped call", bb.cpu().numpy(), n_out.cpu().numpy(),
                   [whole[s][outs(first[s]): outs(counts[s])] for s in range(ns)])

        f.reset()
        bb, n_out = f.baseband_ragged(flat, i64(offs), i32(first), max(first))
        torch.cuda.synchronize()
        check_rows("after reset", bb.cpu().numpy(), n_out.cpu().numpy(), [U.expected(trains[s], h, first[s]) for s in range(ns)])
