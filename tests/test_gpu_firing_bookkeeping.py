"""GPU (-m gpu): a firing's integer bookkeeping in the rotating-window body (csrc/rotwin_body.h, csrc/rot_firing_index.h) against the
oracle, byte for byte and in the loop state it leaves behind: the output ring's byte offset is stepped per symbol and counts the
symbols (the count of a call, the lock events' symbol numbers and first_lock_symbol are put together from it), the clock table's
entry is found by a select cascade on a pre-scaled isub, the sample position advances in place.

The batch is the one of tests/test_gpu_rot_bookkeeping.py (its cases, stream count and sample counts are taken from there):
  * 130 streams: two full waves and a partial one;
  * process_ragged with per-stream sample counts cycling through 0, 1, 7, 8, 9, 63, 64, 65, 79, 80, 81, 200, 733: 733 samples are
    about 229 symbols at 230 kS/s - seven full runs of the 32-symbol ring go out and a partial one is flushed at the end; the short
    counts end inside the first group of 8 symbols and exactly at a group boundary;
  * symbol-clock phases spread over one symbol through set_state, so all four columns of the clock table are read;
  * two chained calls.
Cases: configs[1] s16 / u8 / f32 (the instance with 14 compiled-in steps), 250 kS/s s16 (generic instance, 256-thread blocks),
configs[2] OQPSK - and 60 kS/s for 72 k symbols/s on the same std-window geometry: 1.2 symbols per input sample, so in every fifth
sample the clock fires twice, the earlier symbol is dropped (demod.c:33-47) and the kernel takes the ring back by one symbol -
recomputing the byte offset, also right behind a flush.  The CPU half of that case holds the design to the oracle alone: fed one
sample at a time, the oracle's clock phase falls by two thresholds inside single samples.

Compared per stream and call: soft bytes, symbols_this_call, the lock events with their symbol numbers; after the second call the
state, word by word."""
from __future__ import annotations

import math

import numpy as np
import pytest

import oracle_py as O
from meteor_demod_amd import DemodConfig, Demodulator, synth
from test_gpu_clock_table import _planned
from test_gpu_rot_bookkeeping import CASES as ROT_CASES, COUNTS, NS, _DT, _gpu_words, _oracle_words

pytestmark = pytest.mark.gpu

CASES = dict(ROT_CASES)
CASES["60k_s16_two_symbols_in_a_sample"] = (DemodConfig(samplerate=60000), 256, None)
TWO_IN_A_SAMPLE = ("60k_s16_two_symbols_in_a_sample",)


def _double_firings(cfg, iq, phase) -> int:
    """Input samples of `iq` inside which the oracle's clock crosses its threshold twice: fed one sample at a time, the phase after
    the sample is the phase before plus -O steps of the clock word minus 2 pi (and a loop correction far below pi) per firing."""
    ost = O.OracleStream(cfg)
    ost.state.t_phase = float(phase)
    found = 0
    for k in range(len(iq)):
        p0, f0 = float(ost.state.t_phase), float(ost.state.t_freq)
        ost.run(iq[k:k + 1])
        fell = p0 + cfg.interp_factor * f0 - float(ost.state.t_phase)
        firings = round(fell / (2.0 * math.pi))
        if firings >= 2 and abs(fell - 2.0 * math.pi * firings) < 1.0:
            found += 1
    return found


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_phased_two_calls_match_oracle_bytes_events_and_state(name, gpu_device, monkeypatch):
    import torch
    cfg, block, steps = CASES[name]
    monkeypatch.setenv("MDEMOD_LAT", "0")                   # the lane kernels: a context of 130 streams would take the wave-per-stream one
    got_steps, got_block = _planned(cfg, NS)
    assert got_block == block and (steps is None or got_steps == steps), (got_steps, got_block)

    cnt = [[COUNTS[i % 13] for i in range(NS)], [COUNTS[(i + 6) % 13] for i in range(NS)]]
    streams = [synth.make_stream(9900 + i, cfg.samplerate, cfg.symrate, f0_hz=(i % 9 - 4) * 300.0, clock_ppm=(i % 7 - 3) * 20.0,
                                 esn0_db=14.0, rms=5000.0, oqpsk=cfg.oqpsk, fmt=cfg.bps) for i in range(NS)]
    iqs = [synth.generate_host(s, cnt[0][i] + cnt[1][i]).reshape(-1, 2) if cnt[0][i] + cnt[1][i] else np.zeros((0, 2), _DT[cfg.bps])
           for i, s in enumerate(streams)]
    phases = [np.float32(2.0 * math.pi * 0.98 * i / NS) for i in range(NS)]

    if name in TWO_IN_A_SAMPLE:
        # stream 12: 733 samples in its first call - the oracle alone says that the event this case is about is there, often
        assert cnt[0][12] == 733
        doubles = _double_firings(cfg, iqs[12][:733], phases[12])
        assert doubles >= 733 // 10, doubles

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
            calls.append((soft, ev))
            pos += n
        want.append((calls, _oracle_words(ost.state)))
    if name in TWO_IN_A_SAMPLE:
        # more than one run of the ring, and nearly a symbol per sample although the clock fires 1.2 times per sample
        assert 700 <= want[12][0][0][0].shape[0] <= 733, want[12][0][0][0].shape

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
                assert sa["lock_events_this_call"][i] == len(w_ev), (name, c, i)
                if w_ev:
                    assert d.lock_events(i) == w_ev, (name, c, i, d.lock_events(i), w_ev)
                assert sa["overflow"][i] == 0, (name, c, i)
        states = d.get_states(0, NS)
    for i in range(NS):
        assert _gpu_words(states[i]) == want[i][1], (name, i, _gpu_words(states[i]), want[i][1])
