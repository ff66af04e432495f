"""GPU (-m gpu): the rare events of a firing in the std rotating-window kernel (W::RARE_ONE_BRANCH, csrc/rotwin_body.h: the short
cabsf's fallback, two symbols in one input sample, the far phase wrap, lock / unlock / turn-round and the lock event's record, all
behind one branch on the OR of their lane masks) against the oracle, byte for byte: soft bytes, symbols_this_call, the lock events
with their symbol numbers, and after the second call the state, word by word.

The batch is the one of tests/test_gpu_rot_bookkeeping.py (130 streams, its sample counts 0 .. 733 through process_ragged, clock phases
spread over a symbol, two chained calls; the instances: configs[1] s16 / u8 / f32, 250 kS/s generic, configs[2]) plus the 60 kS/s case
of tests/test_gpu_firing_bookkeeping.py, in which the clock fires twice inside every fifth input sample.  What is new is what the lanes
of ONE wave (streams 0 .. 63) are fed and where they start:
  * every eighth lane (i % 8 == 1) gets all-zero input: the magnitude of every symbol is 0, which the short square root hands to its
    exact fallback on every firing (and out_im may be -0);
  * every eighth lane (i % 8 == 3) gets full-scale random QPSK (+-32767; 0 / 255 in 8 bits): the gain is driven to its clamp at 0;
    in the float case half of these lanes carry 1e7 instead, so that |alpha * e| exceeds 6 pi on the first symbol - the phase before
    the wrap is then beyond 4 pi whatever it was, which is the far wrap (not reachable from 16-bit input);
  * lane 25 (zero input, 733 samples) starts unlocked with its error one decay step above 85: it locks on its first symbols, in
    firings that also take the magnitude's fallback; lane 11 (full scale) starts unlocked just above 85; lane 12 starts locked
    just above 105 (it unlocks); lane 38 starts a few steps inside +fmax sweeping up and lane 51 (full scale; 1e7 in the float case)
    at -fmax sweeping down (both turn round);
  * the second test leaves 24 symbols of room: lane 25 locks on symbol 31, the firing that fills its ring of 32, so the flush's
    overflow side and the lock event's record run in the same firing.
Every event is asserted from the oracle alone before the GPU is asked."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import demod_instances as M
import oracle_py as O
from meteor_demod_amd import DemodConfig, Demodulator, derive_tables
from meteor_demod_amd import synth
from test_gpu_clock_table import _planned
from test_gpu_firing_bookkeeping import CASES, TWO_IN_A_SAMPLE, _double_firings
from test_gpu_rot_bookkeeping import COUNTS, NS, _DT, _gpu_words, _oracle_words

LANE_ZERO_LOCK, LANE_FULL_LOCK, LANE_UNLOCK, LANE_TURN_UP, LANE_TURN_DOWN = 25, 11, 12, 38, 51
ERR_AT_85 = float(np.float32(85.0) / np.float32(0.999))       # one decay step (pll.c:117 with e = 0) above the lock threshold
ERR_LOCK_ON_31 = 87.74           # zero input: 32 decay steps bring it below 85, 31 do not (asserted below)
FAR_AMPLITUDE = 1.0e7
ROOM = 24


def _zero(i: int) -> bool:
    return i % 8 == 1


def _full(i: int) -> bool:
    return i % 8 == 3


def _far(cfg, i: int) -> bool:
    return cfg.bps == 32 and i % 16 == 3


def _input(cfg, i: int, n: int) -> np.ndarray:
    if n == 0:
        return np.zeros((0, 2), _DT[cfg.bps])
    if _zero(i):
        return np.full((n, 2), 128 if cfg.bps == 8 else 0, dtype=_DT[cfg.bps])
    if _full(i):
        # rectangular random QPSK at the sample format's full scale
        k = (np.arange(n) * cfg.symrate) // cfg.samplerate
        signs = np.random.default_rng(31000 + i).integers(0, 2, size=(int(k[-1]) + 1, 2))[k] * 2 - 1
        if cfg.bps == 8:
            return np.where(signs > 0, 255, 0).astype(np.uint8)
        return (signs * (FAR_AMPLITUDE if _far(cfg, i) else 32767.0)).astype(_DT[cfg.bps])
    st = synth.make_stream(12000 + i, cfg.samplerate, cfg.symrate, f0_hz=(i % 9 - 4) * 300.0, clock_ppm=(i % 7 - 3) * 20.0,
                           esn0_db=14.0, rms=5000.0, oqpsk=cfg.oqpsk, fmt=cfg.bps)
    return synth.generate_host(st, n).reshape(-1, 2)


def _start(cfg, i: int, room_case: bool) -> dict:
    fmax = float(derive_tables(cfg)[1]["pll_fmax"])
    d = M._snapshot(O.OracleStream(cfg))
    d["t_phase"] = float(np.float32(2.0 * math.pi * 0.98 * i / NS))
    if i == LANE_ZERO_LOCK:
        d.update(pll_err=float(np.float32(ERR_LOCK_ON_31 if room_case else ERR_AT_85)))
    elif i == LANE_FULL_LOCK:
        d.update(pll_err=float(np.float32(85.5)))
    elif i == LANE_UNLOCK:
        d.update(locked=1, locked_once=1, first_lock_symbol=0, pll_err=float(np.float32(105.2)))        # one decay step leaves it above 105 whatever the signal
    elif i == LANE_TURN_UP:
        d.update(updown=1, pll_freq=float(np.float32(fmax - 3e-6)))
    elif i == LANE_TURN_DOWN:
        d.update(updown=-1, pll_freq=float(np.float32(-fmax)))
    return d


def _pll_error(ost, trace) -> np.ndarray:
    """pll.c:143-151 from the traced symbols, in float as the reference computes it"""
    lut = np.array(list(ost.consts.tanh_lut), dtype=np.float32)

    def th(v):
        return lut[np.clip(v, np.float32(-16.0), np.float32(15.0)).astype(np.int32) + 16]
    i, q = trace["re"], trace["im"]
    return (th(i) * q).astype(np.float32) - (th(q) * i).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _expected(name: str, room_case: bool = False):
    """Per stream (start state, input of both calls, per call (soft, trace, events), final state words) from the oracle; computed once
    per case and shared."""
    cfg = CASES[name][0]
    cnt = [[COUNTS[i % 13] for i in range(NS)], [COUNTS[(i + 6) % 13] for i in range(NS)]]
    out = []
    for i in range(NS):
        start = _start(cfg, i, room_case)
        iq = _input(cfg, i, cnt[0][i] + cnt[1][i])
        ost = O.OracleStream(cfg)
        s = ost.state
        for f in M._STATE_FIELDS:
            setattr(s, f, start[f])
        calls, pos = [], 0
        for c in range(2):
            n = cnt[c][i]
            if n:
                soft, trace, ev = ost.run(iq[pos:pos + n], want_trace=True)
                e = _pll_error(ost, trace)
            else:
                soft, trace, ev, e = np.zeros((0, 2), np.int8), np.zeros(0, O.TRACE_DTYPE), [], np.zeros(0, np.float32)
            calls.append((soft, trace, ev, e))
            pos += n
        out.append((start, iq, calls, _oracle_words(ost.state), float(ost.consts.pll_alpha), float(ost.consts.pll_fmax)))
    return cnt, out


def _assert_design(name: str, room_case: bool = False) -> None:
    """The oracle alone: the events the case is about are there, in lanes of the first wave."""
    cfg = CASES[name][0]
    cnt, lanes = _expected(name, room_case)
    assert cnt[0][LANE_ZERO_LOCK] == 733 and _zero(LANE_ZERO_LOCK) and cnt[0][LANE_TURN_DOWN] == 733 and _full(LANE_TURN_DOWN) and _full(LANE_FULL_LOCK)
    assert max(LANE_ZERO_LOCK, LANE_FULL_LOCK, LANE_UNLOCK, LANE_TURN_UP, LANE_TURN_DOWN) < 64
    # zero input: every symbol's magnitude is 0
    for i in (1, 9, LANE_ZERO_LOCK):
        tr = lanes[i][2][1][1] if i != LANE_ZERO_LOCK else lanes[i][2][0][1]
        assert len(tr) >= 1 and (tr["re"] == 0).all() and (tr["im"] == 0).all() and (tr["gain"] > 1.0).all(), (name, i)
    # full scale: the gain stands at its clamp on many symbols (not in 8 bits: +-128 is no large signal)
    if cfg.bps != 8:
        tr = lanes[LANE_TURN_DOWN][2][0][1]
        assert np.count_nonzero(tr["gain"] == 0) >= 30, (name, np.count_nonzero(tr["gain"] == 0))
    # lock, unlock, turn-round; the zero-input lane locks in a firing whose magnitude is 0
    ev = lanes[LANE_ZERO_LOCK][2][0][2]
    assert ev and ev[0][1] == 1 and ev[0][0] == (31 if room_case else ev[0][0]) and ev[0][0] <= 31, (name, ev)
    assert lanes[LANE_ZERO_LOCK][2][0][1]["re"][ev[0][0]] == 0
    assert any(locked == 1 for c in (0, 1) for _, locked in lanes[LANE_FULL_LOCK][2][c][2]), name
    assert any(locked == 0 for _, locked in lanes[LANE_UNLOCK][2][0][2]), name
    for i in (LANE_TURN_UP, LANE_TURN_DOWN):
        fmax = np.float32(lanes[i][5])
        assert np.count_nonzero(np.abs(lanes[i][2][0][1]["pll_freq"]) >= fmax) >= 1, (name, i)
    # far wrap: |alpha e| >= 6 pi puts |phase + alpha e| beyond 4 pi for every phase inside (-2 pi, 2 pi)
    if cfg.bps == 32:
        assert _far(cfg, LANE_TURN_DOWN)
        _, _, calls, _, alpha, _ = lanes[LANE_TURN_DOWN]
        a = np.abs(calls[0][3]) * np.float32(alpha)
        assert np.count_nonzero(a >= 6.0 * math.pi) >= 1 and np.isfinite(calls[0][1]["re"]).all(), (name, float(a.max()))
    if name in TWO_IN_A_SAMPLE:
        # a normal lane and the zero-input lane: the clock fires twice inside many single samples
        for i in (LANE_UNLOCK, LANE_ZERO_LOCK):
            assert _double_firings(cfg, lanes[i][1][:733], lanes[i][0]["t_phase"]) >= 733 // 10, (name, i)


@pytest.mark.parametrize("name", list(CASES))
def test_design_holds_in_the_oracle(name):
    """No GPU: the constants above are what they are for."""
    _assert_design(name)
    if name == "c1_s16_lut14":
        _assert_design(name, True)


def _run_call(d, cfg, lanes, cnt_c, pos, room):
    import torch
    offsets, p = [], 3
    for i in range(NS):
        offsets.append(p)
        p += cnt_c[i] + 1
    flat = np.zeros((p + 8, 2), dtype=_DT[cfg.bps])
    for i in range(NS):
        flat[offsets[i]:offsets[i] + cnt_c[i]] = lanes[i][1][pos[i]:pos[i] + cnt_c[i]]
    soft = torch.full((NS, room, 2), 99, dtype=torch.int8, device="cuda")
    d.process_ragged(torch.from_numpy(flat).cuda(), torch.tensor(offsets, dtype=torch.int64).cuda(),
                     torch.tensor(cnt_c, dtype=torch.int32).cuda(), soft)
    torch.cuda.synchronize()
    return soft.cpu().numpy(), d.status_array()


def _start_streams(d, lanes):
    for i in range(NS):
        d.set_state(i, M.to_stream_state(lanes[i][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_rare_events_in_one_wave_match_oracle_bytes_events_and_state(name, gpu_device, monkeypatch):
    cfg, block, steps = CASES[name]
    monkeypatch.setenv("MDEMOD_LAT", "0")                   # the lane kernels: a context of 130 streams would take the wave-per-stream one
    got_steps, got_block = _planned(cfg, NS)
    assert got_block == block and (steps is None or got_steps == steps), (got_steps, got_block)
    _assert_design(name)
    cnt, lanes = _expected(name)
    with Demodulator(cfg, NS) as d:
        assert "v3 rotating register window" in d.kernel_name, d.kernel_name
        _start_streams(d, lanes)
        pos = [0] * NS
        for c in range(2):
            soft, sa = _run_call(d, cfg, lanes, cnt[c], pos, d.max_symbols(max(COUNTS)))
            for i in range(NS):
                pos[i] += cnt[c][i]
                w_soft, _, w_ev, _ = lanes[i][2][c]
                assert sa["symbols_this_call"][i] == w_soft.shape[0], (name, c, i, cnt[c][i])
                assert np.array_equal(soft[i, : w_soft.shape[0]], w_soft), (name, c, i, cnt[c][i])
                assert sa["lock_events_this_call"][i] == len(w_ev), (name, c, i)
                if w_ev:
                    assert d.lock_events(i) == w_ev, (name, c, i, d.lock_events(i), w_ev)
                assert sa["overflow"][i] == 0, (name, c, i)
        states = d.get_states(0, NS)
    for i in range(NS):
        assert _gpu_words(states[i]) == lanes[i][3], (name, i, _gpu_words(states[i]), lanes[i][3])


@pytest.mark.gpu
def test_lock_event_in_the_firing_whose_flush_overflows(gpu_device, monkeypatch):
    name = "c1_s16_lut14"
    cfg, block, steps = CASES[name]
    monkeypatch.setenv("MDEMOD_LAT", "0")
    assert _planned(cfg, NS) == (steps, block)
    _assert_design(name, True)
    cnt, lanes = _expected(name, True)
    assert lanes[LANE_ZERO_LOCK][2][0][2] == [(31, 1)]      # the 32nd symbol: the one that fills the ring
    with Demodulator(cfg, NS) as d:
        assert "v3 rotating register window" in d.kernel_name, d.kernel_name
        _start_streams(d, lanes)
        soft, sa = _run_call(d, cfg, lanes, cnt[0], [0] * NS, ROOM)
        for i in range(NS):
            w_soft, _, w_ev, _ = lanes[i][2][0]
            m = min(ROOM, w_soft.shape[0])
            assert sa["symbols_this_call"][i] == w_soft.shape[0] and sa["overflow"][i] == int(w_soft.shape[0] > ROOM), (i, cnt[0][i])
            assert np.array_equal(soft[i, :m], w_soft[:m]) and (soft[i, m:] == 99).all(), i
            assert sa["lock_events_this_call"][i] == len(w_ev), i
            if w_ev:
                assert d.lock_events(i) == w_ev, (i, d.lock_events(i), w_ev)
        # the second call has room again: no overflow bit travels in the flag word
        soft, sa = _run_call(d, cfg, lanes, cnt[1], cnt[0], d.max_symbols(max(COUNTS)))
        for i in range(NS):
            w_soft, _, w_ev, _ = lanes[i][2][1]
            assert sa["symbols_this_call"][i] == w_soft.shape[0] and sa["overflow"][i] == 0, i
            assert np.array_equal(soft[i, : w_soft.shape[0]], w_soft), i
            assert sa["lock_events_this_call"][i] == len(w_ev), i
        states = d.get_states(0, NS)
    for i in range(NS):
        assert _gpu_words(states[i]) == lanes[i][3], (i, _gpu_words(states[i]), lanes[i][3])
