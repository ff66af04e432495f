"""GPU (-m gpu): every compiled demodulator kernel instance (one row of tests/demod_instances.py each) through lock, unlock and relock,
bit for bit against the oracle.

Outside the std window the geometry tests never reach a locked loop (a cold lock takes 2 500 symbols and more); here the oracle runs
the lead-in on the CPU and every lane starts from the oracle's loop state and filter history (mdemod_set_state /
mdemod_set_history) 256 symbols before a transition.  70 lanes; lane i takes (stream, window) pair i mod 20 of five streams x
{ lock, unlock, relock, control }, so neighbouring lanes reach the branch that stores a lock event at different symbols, control
lanes never do, and the lengths are ragged.  The window goes in as chained ragged calls of 1, 3, 64 samples and the rest.
tests/test_demod_instances_host.py checks on the CPU that every row's windows do hold their transitions."""
from __future__ import annotations

import numpy as np
import pytest

import demod_instances as M
from meteor_demod_amd import Demodulator

pytestmark = pytest.mark.gpu

STATE_FLOATS = (("agc_gain", "gain"), ("agc_bias_re", "bias_re"), ("agc_bias_im", "bias_im"), ("pll_phase", "pll_phase"), ("pll_freq", "pll_freq"),
                ("pll_err", "pll_err"), ("t_phase", "t_phase"), ("t_freq", "t_freq"), ("t_prev", "t_prev"), ("oqpsk_inphase", "inphase"))
STATE_INTS = (("pll_locked", "locked"), ("pll_locked_once", "locked_once"), ("pll_updown", "updown"), ("t_dual_state", "dual_state"),
              ("n_samples", "n_samples"), ("n_symbols", "n_symbols"), ("first_lock_symbol", "first_lock_symbol"))


@pytest.mark.parametrize("label", [r.label for r in M.ROWS])
def test_instance_matches_oracle_through_lock_unlock_relock(label, gpu_device, monkeypatch):
    import torch
    row = M.BY_LABEL[label]
    cfg = row.cfg
    for k in ("MDEMOD_LAT", "MDEMOD_KERNEL", "MDEMOD_NO_CLOCK_JUMP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)

    # the oracle's side: five clips, four windows each, every window run in pieces
    pairs = []
    for k, segs in enumerate(M.make_streams(row)):
        iq = M.clip_device(segs)
        _, wins = M.find_windows(cfg, k, iq)
        assert all(w is not None for w in wins), (label, k)
        pairs += [(iq, M.expect(cfg, iq, w)) for w in wins]
    assert len(pairs) == M.N_STREAMS * len(M.KINDS) == 20
    assert sum(len(ev) for _, w in pairs for _, ev in w.calls) >= 15           # (the CPU module holds each window to its transition)

    lanes = [pairs[i % len(pairs)] for i in range(M.LANES)]
    lens = [w.b - w.a for _, w in lanes]
    offsets, pos = [], 3                                                       # odd, unaligned starts
    for n in lens:
        offsets.append(pos)
        pos += n + 1
    flat = np.zeros((pos + 64, 2), dtype=lanes[0][0].dtype)
    for o, (iq, w) in zip(offsets, lanes):
        flat[o:o + w.b - w.a] = iq[w.a:w.b]

    with Demodulator(cfg, M.LANES) as d:
        assert row.name in d.kernel_name, d.kernel_name
        hpad = d.history_len()
        for i, (iq, w) in enumerate(lanes):
            seed = M.decode(iq[w.a - hpad:w.a])
            assert np.array_equal(seed[hpad - (cfg.taps - 1):], w.history[1:])         # the oracle's own history, and what lies before it
            d.set_state(i, M.to_stream_state(w.state))
            d.set_history(i, seed)
        x = torch.from_numpy(flat).cuda()
        soft = torch.zeros((M.LANES, d.max_symbols(max(lens)), 2), dtype=torch.int8, device="cuda")
        first_lock = [w.state["first_lock_symbol"] for _, w in lanes]
        done = [0] * M.LANES
        for c in range(len(M.CHAIN) + 1):
            counts = [M.chain_lengths(n)[c] for n in lens]
            d.process_ragged(x, torch.tensor([o + k for o, k in zip(offsets, done)], dtype=torch.int64).cuda(),
                             torch.tensor(counts, dtype=torch.int32).cuda(), soft)
            torch.cuda.synchronize()
            st = d.status_array()
            got = soft.cpu().numpy()
            for i, (_, w) in enumerate(lanes):
                want, ev = w.calls[c]
                where = (label, i, w.kind, c)
                assert st["symbols_this_call"][i] == len(want) and st["overflow"][i] == 0, where
                assert np.array_equal(got[i, :len(want)], want), where
                assert st["lock_events_this_call"][i] == len(ev) and d.lock_events(i) == ev, (where, d.lock_events(i), ev)
                if first_lock[i] < 0 and any(e[1] for e in ev):
                    first_lock[i] = next(e[0] for e in ev if e[1])
                assert st["first_lock_symbol"][i] == first_lock[i], where
                done[i] += counts[i]
        states = d.get_states(0, M.LANES)
        for i, (_, w) in enumerate(lanes):
            g, s = states[i], w.final
            for a, b in STATE_FLOATS:
                assert np.float32(getattr(g, a)) == np.float32(s[b]), (label, i, w.kind, a, getattr(g, a), s[b])
            for a, b in STATE_INTS:
                assert getattr(g, a) == s[b], (label, i, w.kind, a, getattr(g, a), s[b])
            if w.kind == "lock":
                assert w.state["first_lock_symbol"] == -1 and g.first_lock_symbol == w.event[0]
            assert np.array_equal(d.get_history(i)[-(cfg.taps - 1):], w.final_history[-(cfg.taps - 1):]), (label, i, w.kind)
