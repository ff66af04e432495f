"""The lock detector's wave-uniform early-out (csrc/demod_device.h: md_pll_update_packed<., true>; csrc/pll_flags.h) on the GPU, byte for
byte against the oracle: soft symbols, the final pll_freq / pll_err / flags / first_lock_symbol, and the lock-event lists.

128 streams x 4 096 samples = two waves, so the path without an event and the path with one both run in one launch.  Events are forced
through the state a caller may set (mdemod_set_state), and the oracle's streams start from the same state:
  (a) wave 0: one lane unlocked with err just above 85 (it locks), one lane locked with err just below 105 and a gain that leaves the
      constellation too large (it unlocks); the other 62 lanes far from both thresholds;
  (b) wave 1: one unlocked lane a few 1e-6 steps inside +fmax sweeping up, one at -fmax sweeping down (both turn round); the other 62
      lanes far from everything;
  (c) a control launch: no lane near any threshold.
The first test needs no GPU: it holds the constants below to what they are for - in the oracle alone the designed lanes lock, unlock
and turn round inside the block, and no other lane of either launch has an event or reaches +-fmax."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import demod_instances as M
import oracle_py as O
from meteor_demod_amd import DemodConfig, Demodulator, derive_tables, synth

N_STREAMS, N_SAMPLES, N_CLIPS = 128, 4096, 8

SETTINGS = {
    "configs[1]": (DemodConfig(samplerate=230000), "v3 rotating register window"),
    "configs[2]": (DemodConfig(samplerate=230000, symrate=80000, oqpsk=True), "v3 rotating register window"),
    "packed 1.024 MS/s": (DemodConfig(samplerate=1024000), "v3 rotating packed window, mid"),
}

# ---- the design: constants chosen with the oracle on the CPU (test_design_holds_in_the_oracle keeps them honest) ----------------------
RMS = 300.0                      # complex rms of the clips in LSB (s16), Es/N0 20 dB
SEED0 = 7100                     # clip k: seed SEED0 + 16 k, carrier offset 25 Hz * (k - 3)
AGC_TARGET = 190.0               # agc.c:22
LANE_LOCK, LANE_UNLOCK = 5, 41               # wave 0
LANE_TURN_UP, LANE_TURN_DOWN = 64 + 9, 64 + 50   # wave 1
ERR_LOCK = 85.5                  # unlocked, just above 85: with the gain at GAIN_LOW * nominal |e| stays well below 85 and err falls
ERR_UNLOCK = 104.5               # locked, just below 105: with the gain at GAIN_HIGH * nominal |e| is far above 105 and err rises
GAIN_LOW, GAIN_HIGH = 0.4, 2.5
ERR_FAR_UNLOCKED = 1000.0        # decays to 277 in 1 300 symbols: never below 85
ERR_FAR_LOCKED = 0.0             # rises to 0.73 * mean|e| (about 100 at the AGC's target): never above 105
TURN_STEPS_INSIDE = 3            # LANE_TURN_UP starts at fmax - 3e-6


def _clip(cfg, k: int) -> np.ndarray:
    st = synth.make_stream(SEED0 + 16 * k, cfg.samplerate, cfg.symrate, f0_hz=25.0 * (k - 3), esn0_db=20.0, rms=RMS, oqpsk=cfg.oqpsk, fmt=16)
    return synth.generate_host(st, N_SAMPLES)


@functools.lru_cache(maxsize=None)
def _nominal_gain(name: str) -> float:
    """The gain at which clip 0 sits at the AGC's target: a fresh oracle run over the clip, the gain it ends with."""
    cfg = SETTINGS[name][0]
    ost = O.OracleStream(cfg)
    ost.run(_clip(cfg, 0))
    return float(np.float32(ost.state.gain))


def _lane_state(name: str, launch: str, lane: int) -> dict:
    cfg = SETTINGS[name][0]
    fmax = float(derive_tables(cfg)[1]["pll_fmax"])
    d = M._snapshot(O.OracleStream(cfg))
    g0 = _nominal_gain(name)
    d["gain"] = float(np.float32(g0))
    if lane % 2 == 0:
        d.update(locked=0, locked_once=0, pll_err=float(np.float32(ERR_FAR_UNLOCKED + lane)))
    else:
        d.update(locked=1, locked_once=1, first_lock_symbol=0, pll_err=float(np.float32(ERR_FAR_LOCKED)))
    if launch == "events":
        if lane == LANE_LOCK:
            d.update(locked=0, locked_once=0, first_lock_symbol=-1, pll_err=float(np.float32(ERR_LOCK)), gain=float(np.float32(g0 * GAIN_LOW)))
        elif lane == LANE_UNLOCK:
            d.update(locked=1, locked_once=1, first_lock_symbol=0, pll_err=float(np.float32(ERR_UNLOCK)), gain=float(np.float32(g0 * GAIN_HIGH)))
        elif lane == LANE_TURN_UP:
            d.update(locked=0, locked_once=0, first_lock_symbol=-1, pll_err=float(np.float32(ERR_FAR_UNLOCKED)), updown=1,
                     pll_freq=float(np.float32(fmax - TURN_STEPS_INSIDE * 1e-6)))
        elif lane == LANE_TURN_DOWN:
            d.update(locked=0, locked_once=0, first_lock_symbol=-1, pll_err=float(np.float32(ERR_FAR_UNLOCKED)), updown=-1,
                     pll_freq=float(np.float32(-fmax)))
    return d


def _apply(ost: O.OracleStream, d: dict) -> None:
    s = ost.state
    for f in M._STATE_FIELDS:
        setattr(s, f, d[f])
    s.bias.re, s.bias.im = d["bias_re"], d["bias_im"]


@functools.lru_cache(maxsize=None)
def _expected(name: str, launch: str):
    """Per lane (start state, soft, lock events, final state, symbols at +-fmax, symbols where `locked` flipped) from the oracle; the
    clips.  Computed once per setting and launch and shared by the tests."""
    cfg = SETTINGS[name][0]
    fmax = np.float32(derive_tables(cfg)[1]["pll_fmax"])
    clips = [_clip(cfg, k) for k in range(N_CLIPS)]
    lanes = []
    for i in range(N_STREAMS):
        start = _lane_state(name, launch, i)
        ost = O.OracleStream(cfg)
        _apply(ost, start)
        soft, trace, ev = ost.run(clips[i % N_CLIPS], want_trace=True)
        at_fmax = int(np.count_nonzero(np.abs(trace["pll_freq"]) >= fmax))
        flips = int(np.count_nonzero(np.diff(np.concatenate(([start["locked"]], trace["locked"])))))
        lanes.append((start, soft, ev, M._snapshot(ost), at_fmax, flips))
    return clips, lanes


@pytest.mark.parametrize("name", list(SETTINGS))
def test_design_holds_in_the_oracle(name):
    _, ev_lanes = _expected(name, "events")
    _, ctl_lanes = _expected(name, "control")
    designed = (LANE_LOCK, LANE_UNLOCK, LANE_TURN_UP, LANE_TURN_DOWN)
    start, _, ev, final, _, flips = ev_lanes[LANE_LOCK]
    assert any(locked == 1 for _, locked in ev) and flips >= 1 and final["first_lock_symbol"] >= 0 and start["first_lock_symbol"] == -1, (name, ev)
    _, _, ev, _, _, flips = ev_lanes[LANE_UNLOCK]
    assert any(locked == 0 for _, locked in ev) and flips >= 1, (name, ev)
    for lane, updown0 in ((LANE_TURN_UP, 1), (LANE_TURN_DOWN, -1)):
        start, _, _, final, at_fmax, _ = ev_lanes[lane]
        assert start["updown"] == updown0 and at_fmax >= 1, (name, lane, at_fmax)
    assert ev_lanes[LANE_TURN_UP][3]["updown"] != 1 or ev_lanes[LANE_TURN_UP][4] >= 2, name         # it did turn (or has turned back since)
    # nobody else, and nobody at all in the control launch, has an event or stands at +-fmax
    for lanes, skip in ((ev_lanes, designed), (ctl_lanes, ())):
        for i, (_, soft, ev, _, at_fmax, flips) in enumerate(lanes):
            if i not in skip:
                assert not ev and flips == 0 and at_fmax == 0, (name, i, ev, at_fmax)
            assert len(soft) > 1000 // (4 if name.startswith("packed") else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETTINGS))
def test_early_out_matches_oracle_with_and_without_events(name, gpu_device, monkeypatch):
    import torch
    cfg, kernel = SETTINGS[name]
    for k in ("MDEMOD_KERNEL", "MDEMOD_NO_CLOCK_JUMP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MDEMOD_LAT", "0")                # the lane-per-stream kernels (128 streams alone would take the wave kernel)
    test_design_holds_in_the_oracle(name)
    for launch in ("events", "control"):
        clips, lanes = _expected(name, launch)
        x = torch.from_numpy(np.stack([clips[i % N_CLIPS] for i in range(N_STREAMS)])).cuda()
        with Demodulator(cfg, N_STREAMS) as d:
            assert kernel in d.kernel_name, d.kernel_name
            zeros = np.zeros((d.history_len(), 2), dtype=np.float32)
            for i, (start, *_) in enumerate(lanes):
                d.set_state(i, M.to_stream_state(start))
                d.set_history(i, zeros)
            soft = d.process(x)
            torch.cuda.synchronize()
            st = d.status_array()
            got = soft.cpu().numpy()
            states = d.get_states(0, N_STREAMS)
            for i, (start, want, ev, final, _, _) in enumerate(lanes):
                where = (name, launch, i)
                assert st["symbols_this_call"][i] == len(want) and st["overflow"][i] == 0, where
                assert np.array_equal(got[i, :len(want)], want), where
                assert st["lock_events_this_call"][i] == len(ev) and d.lock_events(i) == ev, (where, d.lock_events(i), ev)
                g = states[i]
                for a, b in (("pll_freq", "pll_freq"), ("pll_err", "pll_err"), ("pll_phase", "pll_phase")):
                    assert np.float32(getattr(g, a)) == np.float32(final[b]), (where, a, getattr(g, a), final[b])
                for a, b in (("pll_locked", "locked"), ("pll_locked_once", "locked_once"), ("pll_updown", "updown"), ("first_lock_symbol", "first_lock_symbol")):
                    assert getattr(g, a) == final[b], (where, a, getattr(g, a), final[b])
                assert st["first_lock_symbol"][i] == final["first_lock_symbol"], where
