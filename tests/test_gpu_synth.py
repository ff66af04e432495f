"""The synthetic source and the truth check on the GPU (csrc/synth.hip), the instrument every other GPU test, smoke() and
bench.py start from: the device generator bit for bit against the host generator (which tests/test_synth_host.py holds against
the signal model), truth_probe_kernel and truth_count_kernel exactly against the numpy counts of tests/synth_ref.py, and the
state machine of synth.truth_check on arrays whose relation to the transmitted symbols is known by construction."""
from __future__ import annotations

import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import synth_ref as R
from meteor_demod_amd import synth

pytestmark = pytest.mark.gpu

FS, RS = 230000.0, 72000.0
RAMPS = ((0.0, 0.0), (40.0, 0.5), (-300.0, -3.0))                      # (Doppler Hz/s, clock ppm/s)
RMS = {8: 60.0, 16: 6000.0, 32: 0.5}
CANARY = 0xA5


def _torch():
    import torch
    return torch


def _streams(fmt, oqpsk, ramp, ns, seed0=500):
    return [synth.make_stream(seed0 + 17 * i, FS, RS, f0_hz=-900.0 + 450.0 * i, clock_ppm=7.0 * i - 10.0, oqpsk=oqpsk, fmt=fmt,
                              rms=RMS[fmt], esn0_db=9.0, doppler_hz_per_s=ramp[0] * (1 + i), clock_ppm_per_s=ramp[1] * (1 + i))
            for i in range(ns)]


# ---- device generator == host generator ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n0", (0, (1 << 32) - 1000, 6_074_000_500, (1 << 40) + 3))
@pytest.mark.parametrize("fmt", (8, 16, 32))
def test_device_equals_host_bit_for_bit(gpu_device, fmt, n0):
    """Ramps (the device's own 64-bit high multiply), noise, n0 != 0, n across 2^32 and beyond the 64-bit triangle."""
    for oqpsk, ramp, count, ns in itertools.product((False, True), RAMPS, (1, 255, 4099), (1, 5)):
        streams = _streams(fmt, oqpsk, ramp, ns)
        dev = synth.generate_device(streams, count, n0=n0).cpu().numpy()
        assert dev.shape == (ns, count, 2)
        for i, st in enumerate(streams):
            assert np.array_equal(dev[i], synth.generate_host(st, count, n0=n0)), (fmt, n0, oqpsk, ramp, count, ns, i)


def test_device_equals_host_when_the_grid_strides(gpu_device):
    """300 x 4099 items are more than the 4096 x 256 threads of the launch: some threads take a second item."""
    ns, count, n0 = 300, 4099, 6_074_000_500
    assert ns * count > 4096 * 256
    streams = [synth.make_stream(9000 + i, FS, RS, f0_hz=(i % 13 - 6) * 300.0, clock_ppm=(i % 7 - 3) * 9.0, oqpsk=bool(i & 1),
                                 doppler_hz_per_s=(i % 5 - 2) * 50.0, clock_ppm_per_s=(i % 5 - 2) * 0.6) for i in range(ns)]
    dev = synth.generate_device(streams, count, n0=n0).cpu().numpy()
    for i, st in enumerate(streams):
        assert np.array_equal(dev[i], synth.generate_host(st, count, n0=n0)), i


@pytest.mark.parametrize("fmt", (8, 16, 32))
def test_strided_output_stays_inside_its_rows(gpu_device, fmt):
    torch = _torch()
    ns, count, pad, guard = 3, 1001, 37, 64
    tdt = {8: torch.uint8, 16: torch.int16, 32: torch.float32}[fmt]
    row = 2 * (count + pad) * (fmt // 8)
    flat = torch.full((guard + ns * row + guard,), CANARY, dtype=torch.uint8, device="cuda")
    view = flat[guard:guard + ns * row].view(tdt).view(ns, count + pad, 2)[:, :count]
    assert not view.is_contiguous() and view.stride(0) > 2 * count
    streams = _streams(fmt, True, RAMPS[1], ns)
    assert synth.generate_device(streams, count, out=view, n0=777).data_ptr() == view.data_ptr()
    got = flat.cpu().numpy()
    assert np.all(got[:guard] == CANARY) and np.all(got[-guard:] == CANARY)
    rows = got[guard:-guard].reshape(ns, row)
    used = 2 * count * (fmt // 8)
    assert np.all(rows[:, used:] == CANARY)
    for i, st in enumerate(streams):
        assert np.array_equal(rows[i, :used], synth.generate_host(st, count, n0=777).view(np.uint8).reshape(-1)), i


def test_empty_generation_writes_nothing(gpu_device):
    torch = _torch()
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    streams = _streams(16, False, RAMPS[0], 2)
    arr = (synth.SynthStream * 2)(*streams)
    for ns, count in ((0, 100), (2, 0), (0, 0)):
        rc = synth.lib().mdemod_synth_device(C.byref(synth.tables()), arr, ns, 5, count, C.c_void_p(buf.data_ptr()), 100, gpu_device)
        assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())


# ---- truth kernels -------------------------------------------------------------------------------------------------------------

SEED = 0x5EED5EED1234
PAIRINGS = [(ri, 2, ii, 1 - ri, 3, iq) for ri in (0, 1) for ii in (0, 1) for iq in (0, 1)]      # Q one symbol later: the OQPSK shape


def _at_odd_offset(soft: np.ndarray):
    """The array on the device, one byte into a larger buffer: (keep-alive tensor, pointer)."""
    torch = _torch()
    buf = torch.full((soft.size + 64,), 85, dtype=torch.int8, device="cuda")
    buf[1:1 + soft.size] = torch.as_tensor(soft.reshape(-1))
    return buf, buf.data_ptr() + 1


def _probe(ptr, m0, count, lag_min, n_lags, device):
    out = np.full((2, 2, max(n_lags, 1)), 0xDEADBEEF, dtype=np.uint32)
    rc = synth.lib().mdemod_synth_truth_probe(SEED, C.c_void_p(ptr), m0, count, lag_min, n_lags, out.ctypes.data, device)
    return rc, out


def _count(ptr, n_symbols, block, hyp, device):
    nb = max((n_symbols + block - 1) // block if block else 1, 1)
    out = np.full((2, nb), 0xDEADBEEF, dtype=np.uint32)
    rc = synth.lib().mdemod_synth_truth_count(SEED, C.c_void_p(ptr), n_symbols, block, (C.c_int32 * 6)(*hyp), out.ctypes.data, device)
    return rc, out


@pytest.mark.parametrize("pairing", PAIRINGS, ids=lambda p: "".join(map(str, p)))
def test_probe_kernel_counts_exactly(gpu_device, pairing):
    soft = R.soft_from(SEED, 777 + 16389, *pairing, magnitudes=sum(pairing))
    keep, ptr = _at_odd_offset(soft)
    rail_i, lag_i, inv_i, rail_q, lag_q, inv_q = pairing
    for m0, count, (lag_min, n_lags) in itertools.product((0, 1, 777), (1, 63, 64, 255, 256, 257, 16389),
                                                          ((-40, 81), (0, 1), (-3, 256), (-1000, 5))):
        rc, got = _probe(ptr, m0, count, lag_min, n_lags, gpu_device)
        assert rc == 0
        want = R.probe_counts(SEED, soft, m0, count, lag_min, n_lags)
        assert np.array_equal(got, want), (m0, count, lag_min, n_lags)
        if lag_min == -1000 and m0 == 0 and count < 996:
            assert not got.any()                                   # before the first transmitted symbol: skipped
        if lag_min == -40:                                         # and by hand: the pairing it was built with
            assert got[0, rail_i, lag_i + 40] == (0 if inv_i else count) and got[1, rail_q, lag_q + 40] == (0 if inv_q else count)
    del keep


def test_probe_refusals(gpu_device):
    keep, ptr = _at_odd_offset(R.soft_from(SEED, 300, *PAIRINGS[0]))
    for count, n_lags in ((100, 0), (100, 257), (0, 81), (100, -1)):
        rc, out = _probe(ptr, 0, count, -40, n_lags, gpu_device)
        assert rc == -1 and np.all(out == 0xDEADBEEF)
    del keep


BUILT = ((0, 0, 0, 1, 0, 0), (1, -40, 1, 0, 1, 0), (0, 0, 1, 1, 1, 1))
HYPS = [(ri, li, ii, 1 - ri, lq, iq) for ri in (0, 1) for ii in (0, 1) for iq in (0, 1)
        for li, lq in ((-40, -40), (0, 0), (1, 1), (0, 1), (-40, 1))]


@pytest.mark.parametrize("built", BUILT, ids=lambda p: "_".join(map(str, p)))
def test_count_kernel_counts_exactly(gpu_device, built):
    assert built in HYPS
    base = R.soft_from(SEED, 3 * 16384 + 17, *built, magnitudes=7)
    for block in (1, 64, 100, 256, 16384):
        for n in (1, 255, 256, 257, 3 * block + 17):
            nb = (n + block - 1) // block
            b = min(1, nb - 1)
            first, last = b * block, min((b + 1) * block, n) - 1
            flips = {(0, 0), (first, 0), (last, 1), (n - 1, 0), (n - 1, 1)}         # (symbol, rail); symbol 0 has j < 0 at lag -40
            soft = base[:n]
            for rail in (0, 1):
                soft = R.flip(soft, sorted(s for s, r in flips if r == rail), rail)
            keep, ptr = _at_odd_offset(soft)
            for hyp in HYPS:
                rc, got = _count(ptr, n, block, hyp, gpu_device)
                assert rc == 0
                ei, eq = R.error_counts(SEED, soft, n, block, hyp)
                assert np.array_equal(got[0], ei) and np.array_equal(got[1], eq), (block, n, hyp)
            # by hand, under the pairing it was built with: the flips whose transmitted symbol exists, and nothing else
            hand = np.zeros((2, nb), dtype=np.uint32)
            for s, r in flips:
                if s + built[3 * r + 1] >= 0:
                    hand[r, s // block] += 1
            rc, got = _count(ptr, n, block, built, gpu_device)
            assert rc == 0 and np.array_equal(got, hand), (block, n)
            del keep


def test_count_refusals(gpu_device):
    keep, ptr = _at_odd_offset(R.soft_from(SEED, 300, *BUILT[0]))
    for n, block in ((0, 64), (300, 0), (0, 0)):
        rc, out = _count(ptr, n, block, BUILT[0], gpu_device)
        assert rc == -1 and np.all(out == 0xDEADBEEF)
    del keep


# ---- synth.truth_check on constructed arrays -----------------------------------------------------------------------------------

BLOCK = 1024
M = 40 * BLOCK + 37
P0 = (0, 3, 0, 1, 3, 1)                     # rx I <- tx I at lag 3; rx Q <- tx Q at lag 3, inverted
RX_I, RX_Q = {"tx_rail": "I", "lag": 3, "inverted": False}, {"tx_rail": "Q", "lag": 3, "inverted": True}


@functools.lru_cache(maxsize=None)
def _stream():
    return synth.make_stream(SEED, FS, RS)


@functools.lru_cache(maxsize=None)
def _clean():
    a = R.soft_from(SEED, M, *P0, magnitudes=11)
    a.setflags(write=False)
    return a


def _check(soft: np.ndarray, device, **kw):
    torch = _torch()
    kw.setdefault("block", BLOCK)
    return synth.truth_check(_stream(), torch.from_numpy(np.array(soft, copy=True)).cuda(), device=device, **kw)


def _quiet(res):
    return res["pairing_changes"] == 0 and res["changes"] == [] and res["unresolved_blocks"] == 0 and res["blocks_not_reached"] == 0


def test_truth_check_clean(gpu_device):
    res = _check(_clean(), gpu_device)
    assert res["symbols_compared"] == M and res["first_symbol_compared"] == 0 and res["rail_decisions_wrong"] == 0
    assert res["rail_error_rate"] == 0.0 and res["worst_block_error_rate"] == 0.0 and res["block_symbols"] == BLOCK
    assert res["pairing_rx_i"] == RX_I and res["pairing_rx_q"] == RX_Q and _quiet(res)


def test_truth_check_counts_scattered_errors(gpu_device):
    rng = np.random.default_rng(2)
    per = np.zeros((2, 41), dtype=np.int64)
    soft = _clean()
    # 15 on the I rail of block 7 (1.5 %), the other 42 anywhere in the whole blocks but there
    rest = rng.choice(np.setdiff1d(np.arange(40 * BLOCK), np.arange(7 * BLOCK, 8 * BLOCK)), 42, replace=False)
    where = {0: np.concatenate([7 * BLOCK + rng.choice(BLOCK, 15, replace=False), rest[:20]]), 1: rest[20:]}
    for rail, s in where.items():
        soft = R.flip(soft, s, rail)
        np.add.at(per[rail], s // BLOCK, 1)
    assert per.sum() == 57 and per.max() == 15 and per.max() < 0.02 * BLOCK
    res = _check(soft, gpu_device)
    assert res["rail_decisions_wrong"] == 57 and res["symbols_compared"] == M and _quiet(res)
    assert res["rail_error_rate"] == 57 / (2 * M) and res["worst_block_error_rate"] == 15 / BLOCK


def test_truth_check_counts_a_bad_block_under_the_same_pairing(gpu_device):
    rng = np.random.default_rng(3)
    k = 31                                                                   # 3 % of a block, above the 2 % that asks for a probe
    soft = R.flip(_clean(), 12 * BLOCK + rng.choice(BLOCK, k, replace=False), 0)
    soft = R.flip(soft, [5 * BLOCK, 30 * BLOCK + 1], 1)
    res = _check(soft, gpu_device)
    assert res["rail_decisions_wrong"] == k + 2 and res["symbols_compared"] == M and _quiet(res)
    assert res["worst_block_error_rate"] == k / BLOCK


def test_truth_check_sees_a_quarter_turn(gpu_device):
    h = 20 * BLOCK
    res = _check(R.rotate_from(SEED, _clean(), h, *P0), gpu_device)
    assert res["pairing_changes"] == 1
    assert res["changes"] == [{"block": 20, "symbol": h, "rx_i": (1, 3, 0), "rx_q": (0, 3, 0)}]
    assert res["pairing_rx_i"] == RX_I and res["pairing_rx_q"] == RX_Q
    assert res["rail_decisions_wrong"] == 0 and res["symbols_compared"] == M
    assert res["unresolved_blocks"] == 0 and res["blocks_not_reached"] == 0


@pytest.mark.parametrize("into", (300, 20))
def test_truth_check_sees_a_symbol_slip(gpu_device, into):
    """A deleted symbol 29 % into a block leaves that block without a pairing; 2 % into it, the block already has the new one."""
    at = 17 * BLOCK + into
    res = _check(R.delete_symbol(_clean(), at), gpu_device)
    assert res["pairing_changes"] == 1 and len(res["changes"]) == 1
    ch = res["changes"][0]
    assert ch["block"] in (17, 18) and ch["symbol"] == ch["block"] * BLOCK
    assert ch["rx_i"] == (0, 4, 0) and ch["rx_q"] == (1, 4, 1)
    assert res["unresolved_blocks"] <= 1 and res["blocks_not_reached"] == 0
    assert res["unresolved_blocks"] == (1 if ch["block"] == 18 else 0)
    assert res["symbols_compared"] == M - 1 - BLOCK * res["unresolved_blocks"]
    # what is wrong is wrong between the slip and the border of its block, and only where that block is compared
    assert res["rail_decisions_wrong"] <= (2 * into if ch["block"] == 17 else 0)


def test_truth_check_rides_out_a_fade(gpu_device):
    lo, hi = 10 * BLOCK + BLOCK // 2, 14 * BLOCK                               # 3.5 blocks
    res = _check(R.randomise(_clean(), lo, hi, seed=4), gpu_device)
    assert res["unresolved_blocks"] in (3, 4)
    assert res["pairing_changes"] == 0 and res["changes"] == [] and res["blocks_not_reached"] == 0
    assert res["rail_decisions_wrong"] == 0 and res["symbols_compared"] == M - BLOCK * res["unresolved_blocks"]


def test_truth_check_edges(gpu_device):
    # first_symbol inside a block: the comparison starts at the next block
    res = _check(_clean(), gpu_device, first_symbol=5 * BLOCK + 1)
    assert res["first_symbol_compared"] == 6 * BLOCK and res["symbols_compared"] == M - 6 * BLOCK
    assert res["rail_decisions_wrong"] == 0 and res["pairing_rx_i"] == RX_I and res["pairing_rx_q"] == RX_Q and _quiet(res)
    # less than one block
    short = R.flip(_clean()[:500], [499], 1)
    res = _check(short, gpu_device)
    assert res["symbols_compared"] == 500 and res["rail_decisions_wrong"] == 1 and res["worst_block_error_rate"] == 1 / 500
    assert res["pairing_rx_i"] == RX_I and res["pairing_rx_q"] == RX_Q and _quiet(res)
    # nothing left to compare
    for first in (M, M + 5 * BLOCK, 40 * BLOCK + 1):
        res = _check(_clean(), gpu_device, first_symbol=first)
        assert res["symbols_compared"] == 0 and res["rail_error_rate"] is None and res["worst_block_error_rate"] is None
        assert res["rail_decisions_wrong"] == 0 and "pairing_rx_i" not in res and _quiet(res)


def test_truth_check_probe_budget(gpu_device):
    noise = np.random.default_rng(5).integers(-128, 128, (300 * BLOCK, 2), dtype=np.int8)
    res = _check(noise, gpu_device, max_probes=256)
    assert res["unresolved_blocks"] == 256 and res["blocks_not_reached"] == 44
    assert res["symbols_compared"] == 0 and res["rail_error_rate"] is None and res["pairing_changes"] == 0


def test_best_pairing_agreement(gpu_device):
    torch = _torch()
    dev = lambda a: torch.from_numpy(np.array(a, copy=True)).cuda()
    m0, count = 1000, 4096
    assert synth.best_pairing_agreement(_stream(), dev(_clean()), m0, count, device=gpu_device) == 1.0
    rng = np.random.default_rng(6)
    for ki, kq in ((37, 12), (5, 41)):
        soft = R.flip(_clean(), m0 + rng.choice(count, ki, replace=False), 0)
        soft = R.flip(soft, m0 + rng.choice(count, kq, replace=False), 1)
        soft = R.flip(soft, [m0 - 1, m0 + count], 0)                           # outside the window: not counted
        assert synth.best_pairing_agreement(_stream(), dev(soft), m0, count, device=gpu_device) == 1.0 - max(ki, kq) / count
    noise = rng.integers(-128, 128, (16384, 2), dtype=np.int8)
    assert abs(synth.best_pairing_agreement(_stream(), dev(noise), 0, 16384, device=gpu_device) - 0.5) <= 0.05
