"""GPU (-m gpu): what the std rotating-window kernel (csrc/rotwin_body.h, csrc/demod_kernel_rot.hip) hands from one call to the next,
against the oracle byte for byte and bit for bit:

  * the four words of the loop state a firing reads and writes once (pll_err, t_prev, the flag word, the sample index of the last
    symbol) live in VGPRs for the whole block (W::REGSLOTS) and go back to the per-stream state at its end;
  * the 64-pair history: the last 64 samples of (old history ++ block), written in place at the end of a block and read into the
    window at the start of the next.

130 streams are two full waves and two lanes (the last wave is mostly parked lanes).  Three chained calls through process_ragged
with per-stream sample counts from COUNTS, in two arrangements: "mixed" shuffles all of them through every wave (lanes that keep
some of their old history next to lanes whose history is the block's alone), "batched" gives every lane at least 64 samples (every
lane of a wave replaces its whole history: the case a wave-wide copy in 16-byte pieces would serve - built and measured as a null,
profiles/r09_state_and_handover.md).  Counts that are no multiple of 4 and a flat buffer whose per-stream offsets are no multiple of
4 samples keep the input off 16-byte boundaries.  After every call: soft symbols, symbol counts, lock-event counts, the whole state
word by word and the history, each against the oracle stream fed the same chunks; then the chain against ONE call on the
concatenation (a second context).

The lock / unlock / relock signal of the golden case c1_fade (input pinned by tests/golden/MANIFEST.json) runs through a chain whose
calls each hold one of the transitions: the flag word and first_lock change while they are held in registers.  A soft buffer smaller
than the symbols produced: the overflow bit travels in the flag word and must not reach the next call."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

import oracle_py as O
from golden_cases import BY_NAME, sha
from meteor_demod_amd import DemodConfig, Demodulator, synth
from test_gpu_clock_table import _planned
from test_gpu_rot_bookkeeping import _gpu_words, _oracle_words

pytestmark = pytest.mark.gpu

NS = 130
KBACK = 64
COUNTS = [0, 1, 5, 63, 64, 65, 67, 128, 131, 1000]
AT_LEAST_KBACK = [c for c in COUNTS if c >= KBACK]
_DT = {8: np.uint8, 16: np.int16, 32: np.float32}

QPSK = dict(samplerate=230000)                                    # configs[1]: <FMT, 0, 14, 0, 1>
OQPSK = dict(samplerate=230000, symrate=80000, oqpsk=True)        # configs[2]: <FMT, 1, 6, 0, 1>
CASES = {f"{mode}_{'s16' if bps == 16 else 'u8' if bps == 8 else 'f32'}": (DemodConfig(bps=bps, **kw), steps)
         for mode, kw, steps in (("qpsk", QPSK, 14), ("oqpsk", OQPSK, 6)) for bps in (16, 8, 32)}


def _counts(arrangement: str) -> list:
    """[call][stream] sample counts.  7 and 5 are coprime to the lengths of the lists: every run of ten (six) lanes holds each count
    once, and the three calls of a stream differ."""
    if arrangement == "mixed":
        return [[COUNTS[(7 * i + 3 * c) % len(COUNTS)] for i in range(NS)] for c in range(3)]
    return [[AT_LEAST_KBACK[(5 * i + c) % len(AT_LEAST_KBACK)] for i in range(NS)] for c in range(3)]


def _signals(cfg, totals, seed0):
    streams = [synth.make_stream(seed0 + i, cfg.samplerate, cfg.symrate, f0_hz=(i % 9 - 4) * 300.0, clock_ppm=(i % 7 - 3) * 20.0,
                                 esn0_db=14.0, rms=0.4 if cfg.bps == 32 else 60.0 if cfg.bps == 8 else 5000.0, oqpsk=cfg.oqpsk, fmt=cfg.bps)
               for i in range(NS)]
    return [synth.generate_host(s, n).reshape(-1, 2) if n else np.zeros((0, 2), _DT[cfg.bps]) for s, n in zip(streams, totals)]


def _oracle_chain(cfg, iq, chunks):
    """Per call: (soft, lock events, state words, history) of one oracle stream fed `chunks` samples at a time."""
    ost = O.OracleStream(cfg)
    out, pos = [], 0
    for n in chunks:
        soft, ev = (np.zeros((0, 2), np.int8), [])
        if n:
            soft, _, ev = ost.run(iq[pos:pos + n])
        pos += n
        out.append((soft, ev, _oracle_words(ost.state), ost.history()[-KBACK:].copy()))
    return out


def _ragged_call(d, cfg, blocks, cap):
    """One process_ragged call: stream i gets blocks[i] ([n_i, 2]) from a flat buffer with odd starts.  Returns (soft, status)."""
    import torch
    offsets, p = [], 3
    for b in blocks:
        offsets.append(p)
        p += b.shape[0] + 1
    flat = np.zeros((p + 8, 2), dtype=_DT[cfg.bps])
    for o, b in zip(offsets, blocks):
        flat[o:o + b.shape[0]] = b
    soft = torch.full((NS, cap, 2), 99, dtype=torch.int8, device="cuda")
    d.process_ragged(torch.from_numpy(flat).cuda(), torch.tensor(offsets, dtype=torch.int64).cuda(),
                     torch.tensor([b.shape[0] for b in blocks], dtype=torch.int32).cuda(), soft)
    torch.cuda.synchronize()
    return soft.cpu().numpy(), d.status_array()


def _check_call(d, tag, soft, sa, want_per_stream):
    """Soft bytes, counts, state and history of every stream after a call against (soft, events, words, history)."""
    states = d.get_states(0, NS)
    for i, (w_soft, w_ev, w_words, w_hist) in enumerate(want_per_stream):
        assert sa["symbols_this_call"][i] == w_soft.shape[0], (tag, i)
        assert np.array_equal(soft[i, : w_soft.shape[0]], w_soft), (tag, i)
        assert sa["lock_events_this_call"][i] == len(w_ev), (tag, i)
        assert sa["overflow"][i] == 0, (tag, i)
        assert _gpu_words(states[i]) == w_words, (tag, i, _gpu_words(states[i]), w_words)
        assert np.array_equal(d.get_history(i)[-KBACK:].view(np.uint32), w_hist.view(np.uint32)), (tag, i)


@pytest.mark.parametrize("arrangement", ["mixed", "batched"])
@pytest.mark.parametrize("name", list(CASES))
def test_three_call_chain_state_and_history_match_oracle_and_one_shot(name, arrangement, gpu_device, monkeypatch):
    cfg, steps = CASES[name]
    monkeypatch.setenv("MDEMOD_LAT", "0")                   # the lane kernels: a context of 130 streams would take the wave-per-stream one
    assert _planned(cfg, NS) == (steps, 512)                # the instance with the sine table and the steps compiled in
    cnt = _counts(arrangement)
    if arrangement == "mixed":                              # lanes below and at or above kBack in every wave, in every call
        assert all(min(c[w:w + 64]) < KBACK <= max(c[w:w + 64]) for c in cnt for w in (0, 64))
    else:
        assert all(min(c) >= KBACK for c in cnt)
    assert any(n % 4 for c in cnt for n in c)
    totals = [sum(c[i] for c in cnt) for i in range(NS)]
    iqs = _signals(cfg, totals, 9900)
    want = [_oracle_chain(cfg, iqs[i], [c[i] for c in cnt]) for i in range(NS)]
    cap = 1000                                              # (more than 1000 samples can make: at least 2.8 samples per symbol)

    with Demodulator(cfg, NS) as d:
        assert "v3 rotating register window" in d.kernel_name, d.kernel_name
        assert d.history_len() == KBACK
        pos, parts = [0] * NS, [[] for _ in range(NS)]
        for c in range(3):
            blocks = [iqs[i][pos[i]:pos[i] + cnt[c][i]] for i in range(NS)]
            soft, sa = _ragged_call(d, cfg, blocks, cap)
            _check_call(d, (name, arrangement, c), soft, sa, [want[i][c] for i in range(NS)])
            for i in range(NS):
                pos[i] += cnt[c][i]
                parts[i].append(soft[i, : sa["symbols_this_call"][i]])
        chain_words = [_gpu_words(s) for s in d.get_states(0, NS)]
        chain_hist = [d.get_history(i) for i in range(NS)]

    # one call on the concatenation
    with Demodulator(cfg, NS) as d:
        soft, sa = _ragged_call(d, cfg, iqs, 3 * cap)
        states = d.get_states(0, NS)
        for i in range(NS):
            whole = np.concatenate(parts[i])
            assert sa["symbols_this_call"][i] == whole.shape[0], (name, arrangement, i)
            assert np.array_equal(soft[i, : whole.shape[0]], whole), (name, arrangement, i)
            assert _gpu_words(states[i]) == chain_words[i], (name, arrangement, i)
            assert np.array_equal(d.get_history(i).view(np.uint32), chain_hist[i].view(np.uint32)), (name, arrangement, i)


def test_lock_unlock_relock_inside_the_chain(gpu_device, monkeypatch):
    """c1_fade (signal / noise only / signal) on lanes 0, 70 and 129, short blocks on every other lane; the second call ends between the
    unlock and the relock, so each call holds one transition."""
    monkeypatch.setenv("MDEMOD_LAT", "0")
    case = BY_NAME["c1_fade"]
    cfg = case.cfg
    meta = json.loads((Path(__file__).parent / "golden" / "MANIFEST.json").read_text())["cases"]["c1_fade"]
    fade = case.generate()
    assert sha(fade) == meta["input_sha256"]
    chunks = [100000, 51000, fade.shape[0] - 151000]        # (unlock near sample 150 030, relock near 151 890: MANIFEST's symbols x 3.19)
    carriers = (0, 70, 129)
    assert _planned(cfg, NS) == (14, 512)
    cnt = [[chunks[c] if i in carriers else COUNTS[(7 * i + 3 * c) % len(COUNTS)] for i in range(NS)] for c in range(3)]
    others = _signals(cfg, [0 if i in carriers else sum(c[i] for c in cnt) for i in range(NS)], 9950)
    iqs = [fade if i in carriers else others[i] for i in range(NS)]
    want_fade = _oracle_chain(cfg, fade, chunks)
    want = [want_fade if i in carriers else _oracle_chain(cfg, iqs[i], [c[i] for c in cnt]) for i in range(NS)]
    # the oracle's own events: lock, unlock, relock, one per call, and they are the reference's (MANIFEST)
    assert [[e[1] for e in call[1]] for call in want_fade] == [[1], [0], [1]]
    assert [list(e) for call in want_fade for e in call[1]] == meta["lock_events"]

    with Demodulator(cfg, NS) as d:
        assert "v3 rotating register window" in d.kernel_name, d.kernel_name
        cap = d.max_symbols(max(chunks))
        pos, events = [0] * NS, {i: [] for i in carriers}
        for c in range(3):
            blocks = [iqs[i][pos[i]:pos[i] + cnt[c][i]] for i in range(NS)]
            soft, sa = _ragged_call(d, cfg, blocks, cap)
            _check_call(d, ("fade", c), soft, sa, [want[i][c] for i in range(NS)])
            for i in range(NS):
                pos[i] += cnt[c][i]
            for i in carriers:
                ev = d.lock_events(i)
                assert [list(e) for e in ev] == [list(e) for e in want_fade[c][1]], (c, i)
                events[i] += ev
        st = d.status()
        for i in carriers:
            assert [list(e) for e in events[i]] == meta["lock_events"], i
            assert st[i].first_lock_symbol == meta["first_lock_symbol"] and st[i].locked == meta["final"]["locked"], i


@pytest.mark.parametrize("name", ["qpsk_s16", "oqpsk_s16"])
def test_soft_cap_below_symbols_produced(name, gpu_device, monkeypatch):
    """40 symbols of room: a lane with 1000 samples fills its ring of 32 once inside the room and crosses its end with the second
    (the overflow bit is set in the flag word in the middle of the block), lanes with few samples stay inside.  Everything but the
    bytes behind the room is as without the limit, and the next call, with room, reports no overflow."""
    cfg, steps = CASES[name]
    monkeypatch.setenv("MDEMOD_LAT", "0")
    assert _planned(cfg, NS) == (steps, 512)
    cnt = _counts("mixed")[:2]
    iqs = _signals(cfg, [cnt[0][i] + cnt[1][i] for i in range(NS)], 9980)
    want = [_oracle_chain(cfg, iqs[i], [cnt[0][i], cnt[1][i]]) for i in range(NS)]
    room = 40
    assert max(w[0][0].shape[0] for w in want) > 2 * room and min(w[0][0].shape[0] for w in want) < room
    with Demodulator(cfg, NS) as d:
        assert "v3 rotating register window" in d.kernel_name, d.kernel_name
        soft, sa = _ragged_call(d, cfg, [iqs[i][: cnt[0][i]] for i in range(NS)], room)
        states = d.get_states(0, NS)
        for i in range(NS):
            w_soft, w_ev, w_words, w_hist = want[i][0]
            m = min(room, w_soft.shape[0])
            assert sa["symbols_this_call"][i] == w_soft.shape[0] and sa["overflow"][i] == int(w_soft.shape[0] > room), i
            assert np.array_equal(soft[i, :m], w_soft[:m]) and (soft[i, m:] == 99).all(), i
            assert sa["lock_events_this_call"][i] == len(w_ev), i
            assert _gpu_words(states[i]) == w_words, (i, _gpu_words(states[i]), w_words)
            assert np.array_equal(d.get_history(i)[-KBACK:].view(np.uint32), w_hist.view(np.uint32)), i
        soft, sa = _ragged_call(d, cfg, [iqs[i][cnt[0][i]:] for i in range(NS)], 1000)
        _check_call(d, (name, "second call"), soft, sa, [want[i][1] for i in range(NS)])
