"""GPU (-m gpu): the bookkeeping of a firing of the std rotating-window kernel (csrc/rotwin_body.h, csrc/demod_kernel_rot.hip) against
the oracle, byte for byte and in the loop state it leaves behind: the FIR's padding bounds from three lane masks read against exec,
the window's rotation and base kept as scalars by the slide's assembly, the end-of-block bound worked out once per lane, the
accumulator zeroed inside the FIR.

What the batch is made to do:
  * 130 streams: two full waves and a partial one - lanes past the last stream are parked from the start, so the firing's masks are
    taken over an exec with holes;
  * process_ragged with per-stream sample counts cycling through 0, 1, 7, 8, 9, 63, 64, 65, 79, 80, 81, 200, 733: lanes finish in
    different loop iterations (and some never start), the longest ones slide more than ten times, so the rotation wraps;
  * symbol-clock phases spread over one symbol (through get_state / set_state, the oracle's state set alike): the smallest and the
    largest alignment of a wave differ and both padding bounds move;
  * two chained calls: history is handed over and rot / base start again from 0.

Compared per stream and call: soft bytes, symbols_this_call, the number of lock events; after the second call the state, word by
word.  Cases: configs[1] s16 (the instance with the sine table and 14 compiled-in steps), the same with 8-bit and float input,
250 kS/s s16 (the generic instance) and configs[2] (OQPSK, 6 compiled-in steps)."""
from __future__ import annotations

import math

import numpy as np
import pytest

import oracle_py as O
from meteor_demod_amd import DemodConfig, Demodulator, synth
from test_gpu_clock_table import _planned

pytestmark = pytest.mark.gpu

NS = 130
COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 79, 80, 81, 200, 733]
_DT = {8: np.uint8, 16: np.int16, 32: np.float32}

# name -> (configuration, threads per block, blind steps of the clock table): 512 threads + the step count = the instance with the
# sine table and the steps compiled in (demod_kernel_rot<.., 14 | 6, 0, 1>), 256 = the generic one
CASES = {
    "c1_s16_lut14": (DemodConfig(samplerate=230000), 512, 14),
    "c1_u8_lut14": (DemodConfig(samplerate=230000, bps=8), 512, 14),
    "c1_f32_lut14": (DemodConfig(samplerate=230000, bps=32), 512, 14),
    "250k_s16_generic": (DemodConfig(samplerate=250000), 256, None),
    "c2_oqpsk_lut6": (DemodConfig(samplerate=230000, symrate=80000, oqpsk=True), 512, 6),
}


def _f32_words(*vals) -> tuple:
    return tuple(int(np.float32(v).view(np.uint32)) for v in vals)


def _oracle_words(s) -> tuple:
    return _f32_words(s.gain, s.bias.re, s.bias.im, s.pll_phase, s.pll_freq, s.pll_err) + (s.locked, s.locked_once, s.updown) + \
        _f32_words(s.t_phase, s.t_freq, s.t_prev) + (s.dual_state,) + _f32_words(s.inphase) + (s.n_samples, s.n_symbols, s.first_lock_symbol)


def _gpu_words(g) -> tuple:
    return _f32_words(g.agc_gain, g.agc_bias_re, g.agc_bias_im, g.pll_phase, g.pll_freq, g.pll_err) + (g.pll_locked, g.pll_locked_once, g.pll_updown) + \
        _f32_words(g.t_phase, g.t_freq, g.t_prev) + (g.t_dual_state,) + _f32_words(g.oqpsk_inphase) + (g.n_samples, g.n_symbols, g.first_lock_symbol)


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_phased_two_calls_match_oracle_bytes_and_state(name, gpu_device, monkeypatch):
    import torch
    cfg, block, steps = CASES[name]
    monkeypatch.setenv("MDEMOD_LAT", "0")                   # the lane kernels: a context of 130 streams would take the wave-per-stream one
    got_steps, got_block = _planned(cfg, NS)
    assert got_block == block and (steps is None or got_steps == steps), (got_steps, got_block)

    # per stream: first call COUNTS[i % 13] samples, second call the count six places on (so every stream gets input and the
    # lanes of a wave finish in another order)
    cnt = [[COUNTS[i % 13] for i in range(NS)], [COUNTS[(i + 6) % 13] for i in range(NS)]]
    streams = [synth.make_stream(9700 + i, cfg.samplerate, cfg.symrate, f0_hz=(i % 9 - 4) * 300.0, clock_ppm=(i % 7 - 3) * 20.0,
                                 esn0_db=14.0, rms=5000.0, oqpsk=cfg.oqpsk, fmt=cfg.bps) for i in range(NS)]
    iqs = [synth.generate_host(s, cnt[0][i] + cnt[1][i]).reshape(-1, 2) if cnt[0][i] + cnt[1][i] else np.zeros((0, 2), _DT[cfg.bps])
           for i, s in enumerate(streams)]
    phases = [np.float32(2.0 * math.pi * 0.98 * i / NS) for i in range(NS)]

    # the oracle, stream by stream: the same phase in its state, the same two blocks
    want = []
    for i in range(NS):
        ost = O.OracleStream(cfg)
        ost.state.t_phase = float(phases[i])
        calls, pos = [], 0
        for c in range(2):
            n = cnt[c][i]
            if n:
                soft, _, ev = ost.run(iqs[i][pos:pos + n])
            else:
                soft, ev = np.zeros((0, 2), np.int8), []
            calls.append((soft, len(ev)))
            pos += n
        want.append((calls, _oracle_words(ost.state)))

    with Demodulator(cfg, NS) as d:
        assert "v3 rotating register window" in d.kernel_name, d.kernel_name
        for i in range(NS):
            st = d.get_state(i)
            st.t_phase = float(phases[i])
            d.set_state(i, st)
        pos = [0] * NS
        for c in range(2):
            # odd, unaligned starts in one flat buffer
            offsets, p = [], 3
            for i in range(NS):
                offsets.append(p)
                p += cnt[c][i] + 1
            flat = np.zeros((p + 8, 2), dtype=_DT[cfg.bps])
            for i in range(NS):
                flat[offsets[i]:offsets[i] + cnt[c][i]] = iqs[i][pos[i]:pos[i] + cnt[c][i]]
                pos[i] += cnt[c][i]
            soft = torch.zeros((NS, d.max_symbols(max(COUNTS)), 2), dtype=torch.int8, device="cuda")
            d.process_ragged(torch.from_numpy(flat).cuda(), torch.tensor(offsets, dtype=torch.int64).cuda(),
                             torch.tensor(cnt[c], dtype=torch.int32).cuda(), soft)
            torch.cuda.synchronize()
            sa = d.status_array()
            soft = soft.cpu().numpy()
            for i in range(NS):
                w_soft, w_ev = want[i][0][c]
                assert sa["symbols_this_call"][i] == w_soft.shape[0], (name, c, i, cnt[c][i])
                assert np.array_equal(soft[i, : w_soft.shape[0]], w_soft), (name, c, i, cnt[c][i])
                assert sa["lock_events_this_call"][i] == w_ev, (name, c, i)
                assert sa["overflow"][i] == 0, (name, c, i)
        states = d.get_states(0, NS)
    for i in range(NS):
        assert _gpu_words(states[i]) == want[i][1], (name, i, _gpu_words(states[i]), want[i][1])
