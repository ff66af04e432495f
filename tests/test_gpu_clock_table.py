"""GPU (-m gpu): the symbol clock's position table in LDS (csrc/rotwin_body.h: rot_clock_fast reads { samples to advance, isub, bank }
at isub * 4 + j instead of dividing by -O) against the oracle, byte for byte and in the loop state it leaves behind.

Every -O of 1, 2, 4, 5, 8 and 16 runs once with 14 blind steps (QPSK) and once with 6 (OQPSK): the sample rate is chosen for the step
count, the planner then picks the kernel.  The instances with the step count compiled in (`demod_kernel_rot<.., 14 | 6, 0, 1>`, the
ones with the sine table: 512-thread blocks) need the std window (at most 3.6 samples per firing) AND 64 KB of LDS next to 5.4 KB of
coefficient rows per bank, so they exist for OQPSK at -O 2, 4, 5 and for QPSK at -O 5 only; the other rates take the same table
through the generic body of whichever window serves them (CASES below says which, and the test checks it).  One configuration
each for the mid packed window and the gather kernel (its jump schedule switched off: with one it keeps the arithmetic), and one
that keeps the arithmetic (3.2 MS/s: jump schedule, no table), which must pass unchanged.

70 streams are a full and a partial wave, 513 cross the 512-thread block.  4 099 samples go in as blocks of 1, 2, 3, 5, 64, 1000 and
3024: a lane whose next firing lies past the block's end leaves the table's path for the stepping loop in the middle of an input
sample (isub != 0 with -O > 1) and the next call's table takes over from the stepping loop."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle_py as O
from meteor_demod_amd import DemodConfig, Demodulator, _capi, synth

pytestmark = pytest.mark.gpu

BLOCKS = [1, 2, 3, 5, 64, 1000, 3024]
N = sum(BLOCKS)
DISTINCT = 70

# name -> (configuration, piece of kernel_name, threads per block, blind steps of the table or None without one, environment)
CASES = {
    "O1_qpsk_14": (DemodConfig(samplerate=1161000, interp_factor=1), "rotating packed window, far", 256, 14, {}),
    "O2_qpsk_14": (DemodConfig(samplerate=580000, interp_factor=2), "rotating packed window, mid", 256, 14, {}),
    "O4_qpsk_14": (DemodConfig(samplerate=290000, interp_factor=4), "rotating packed window, mid", 256, 14, {}),
    "O5_qpsk_14": (DemodConfig(samplerate=230000, interp_factor=5), "v3 rotating register window", 512, 14, {}),          # <16,0,14,0,1>: configs[1]
    "O8_qpsk_14": (DemodConfig(samplerate=137000, interp_factor=8), "v3 rotating register window", 256, 14, {}),
    "O16_qpsk_14": (DemodConfig(samplerate=69000, interp_factor=16), "v3 rotating register window", 256, 14, {}),
    "O1_oqpsk_6": (DemodConfig(samplerate=1301000, symrate=80000, oqpsk=True, interp_factor=1), "rotating packed window, mid", 256, 6, {}),
    "O2_oqpsk_6": (DemodConfig(samplerate=570000, symrate=80000, oqpsk=True, interp_factor=2), "v3 rotating register window", 512, 6, {}),   # <16,1,6,0,1>
    "O4_oqpsk_6": (DemodConfig(samplerate=285000, symrate=80000, oqpsk=True, interp_factor=4), "v3 rotating register window", 512, 6, {}),   # <16,1,6,0,1>
    "O5_oqpsk_6": (DemodConfig(samplerate=230000, symrate=80000, oqpsk=True, interp_factor=5), "v3 rotating register window", 512, 6, {}),   # <16,1,6,0,1>: configs[2]
    "O8_oqpsk_6": (DemodConfig(samplerate=143000, symrate=80000, oqpsk=True, interp_factor=8), "v3 rotating register window", 256, 6, {}),
    "O16_oqpsk_6": (DemodConfig(samplerate=72000, symrate=80000, oqpsk=True, interp_factor=16), "v3 rotating register window", 256, 6, {}),
    "mid_generic": (DemodConfig(samplerate=1024000), "rotating packed window, mid", 256, 69, {}),
    "gather_generic": (DemodConfig(samplerate=6000000), "v3 gather", 256, 412, {"MDEMOD_NO_CLOCK_JUMP": "1"}),
    "keeps_arithmetic_3200k": (DemodConfig(samplerate=3200000), "rotating packed window, far", 256, None, {}),
}

_reference: dict = {}


def _inputs_and_oracle(name):
    """DISTINCT streams of the case and what the oracle makes of each in one go: computed once, shared by both stream counts."""
    if name not in _reference:
        cfg = CASES[name][0]
        streams = [synth.make_stream(9300 + i, cfg.samplerate, cfg.symrate, f0_hz=(i % 9 - 4) * 300.0, clock_ppm=(i % 7 - 3) * 20.0,
                                     esn0_db=14.0, rms=5000.0, oqpsk=cfg.oqpsk, fmt=cfg.bps) for i in range(DISTINCT)]
        iqs = [synth.generate_host(s, N) for s in streams]
        want = []
        for iq in iqs:
            ost = O.OracleStream(cfg)
            soft = ost.run(iq)[0]
            s = ost.state
            want.append((soft, (np.float32(s.t_phase), np.float32(s.t_freq), s.locked, s.locked_once, s.updown, s.dual_state, s.n_symbols,
                                s.n_samples, np.float32(s.pll_phase), np.float32(s.pll_freq), np.float32(s.gain))))
        _reference[name] = (np.stack(iqs), want)
    return _reference[name]


def _planned(cfg, ns):
    """(blind steps of the planned table or None, threads per block) - host arithmetic, what mdemod_create decides."""
    lib = _capi.lib()
    p = cfg.to_c(ns, 0)
    name = C.create_string_buffer(256)
    block = C.c_uint32()
    assert lib.mdemod_plan_kernel(C.byref(p), name, 256, None, C.byref(block)) == 0
    buf = (C.c_int32 * (64 * 16))()
    n = lib.mdemod_plan_clock_table(C.byref(p), buf, 64 * 4)
    assert n >= 0
    if n == 0:
        return None, block.value
    assert n == 4 * cfg.interp_factor
    dv, _, isub_new, _ = buf[0:4]
    return (dv - (isub_new > 0)) * cfg.interp_factor + isub_new - 1, block.value


@pytest.mark.parametrize("ns", [70, 513])
@pytest.mark.parametrize("name", list(CASES))
def test_table_clock_matches_oracle_bytes_and_state(name, ns, gpu_device, monkeypatch):
    import torch
    cfg, kernel, block, steps, env = CASES[name]
    monkeypatch.setenv("MDEMOD_LAT", "0")                   # the lane kernels: a context of 70 streams would take the wave-per-stream one
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    iq, want = _inputs_and_oracle(name)
    assert _planned(cfg, ns) == (steps, block)
    x = torch.from_numpy(iq[np.arange(ns) % DISTINCT]).cuda()
    with Demodulator(cfg, ns) as d:
        assert kernel in d.kernel_name, d.kernel_name
        parts = [[] for _ in range(ns)]
        pos = 0
        for b in BLOCKS:
            soft = d.process(x[:, pos:pos + b].contiguous())
            torch.cuda.synchronize()
            cnt = d.status_array()["symbols_this_call"]
            soft = soft.cpu().numpy()
            for i in range(ns):
                parts[i].append(soft[i, : cnt[i]])
            pos += b
        states = d.get_states(0, ns)
    for i in range(ns):
        w_soft, w_state = want[i % DISTINCT]
        assert np.array_equal(np.concatenate(parts[i]), w_soft), (name, i)
        g = states[i]
        got = (np.float32(g.t_phase), np.float32(g.t_freq), g.pll_locked, g.pll_locked_once, g.pll_updown, g.t_dual_state, g.n_symbols,
               g.n_samples, np.float32(g.pll_phase), np.float32(g.pll_freq), np.float32(g.agc_gain))
        assert got == w_state, (name, i, got, w_state)
