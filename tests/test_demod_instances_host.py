"""CPU: the demodulator's kernel instances as a matrix (tests/demod_instances.py) - every compiled instance has exactly one row,
every row's configuration plans to its instance, and every row's signal takes the oracle through lock, unlock and relock inside the
windows tests/test_gpu_demod_instances.py runs on the GPU (which therefore cannot pass by comparing 0 with 0)."""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

import demod_instances as M

LABELS = [r.label for r in M.ROWS]


@pytest.fixture
def row(request, monkeypatch):
    r = M.BY_LABEL[request.param]
    for k in ("MDEMOD_LAT", "MDEMOD_KERNEL", "MDEMOD_NO_CLOCK_JUMP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    return r


def test_every_compiled_instance_has_exactly_one_row():
    """Entry labels `_Z...demod_kernel...` of the device assembly build() keeps for the five kernel files against the matrix: a new
    instance needs a row, a row needs an instance."""
    compiled = Counter(M.compiled_instances())
    rows = Counter(LABELS)
    assert len(compiled) >= 85 and all(n == 1 for n in compiled.values()), compiled.most_common(3)
    assert sorted(compiled) == sorted(rows), (sorted(set(compiled) - set(rows)), sorted(set(rows) - set(compiled)))
    assert all(n == 1 for n in rows.values()), rows.most_common(3)
    per_family = Counter("demod_kernel_rotp" if lab.startswith("demod_kernel_rotp") else lab.split("<")[0] for lab in compiled)
    assert per_family == {"demod_kernel_rot": 18, "demod_kernel_roth": 8, "demod_kernel_rotp": 13, "demod_kernel_gat": 10,
                          "demod_kernel_lat": 12, "demod_kernel": 24}, per_family


@pytest.mark.parametrize("row", LABELS, indirect=True)
def test_row_plans_to_its_instance(row):
    """mdemod_plan_kernel gives the row's name piece and block size, the words of mdemod_plan_launch lead the launch tables to the
    row's instance, and where the blind steps of the clock table decide they are the row's."""
    name, block, words, steps = M.planned(row)
    assert row.name in name, (row.label, name)
    assert block == row.block, (row.label, block)
    assert M.instance_label(words) == row.label, (row.label, words)
    if row.steps is not None:
        assert steps == row.steps, (row.label, steps)
    assert words[M.P_BPS] == row.cfg.bps and words[M.P_OQPSK] == int(row.cfg.oqpsk)
    assert row.lead_in == "import"                 # no row needed the GPU for its lead-in


@pytest.mark.parametrize("row", LABELS, indirect=True)
def test_every_row_locks_unlocks_and_relocks_in_the_oracle(row):
    """The oracle alone over the row's five clips: each has a lock, an unlock after it and a relock after that, at symbols that
    differ from stream to stream; the three windows around them and one control window without a transition lie inside the clip;
    run in pieces (lead-in, snapshot, the window call by call) the oracle reports each window's transition in the window's last
    call - and none in the control window; the history it hands over is the decoded tail of the lead-in."""
    cfg = row.cfg
    taps = cfg.taps
    at = {k: [] for k in M.KINDS}
    for k, segs in enumerate(M.make_streams(row)):
        iq = M.clip_host(segs)
        events, wins = M.find_windows(cfg, k, iq)
        assert all(w is not None for w in wins), (row.label, k, events[:6], len(iq))
        lock, unlock, relock = M.transitions(events)
        assert lock[0] < unlock[0] < relock[0]
        for w in wins:
            assert 0 < w.a < w.b <= len(iq) and w.a >= 256 and w.b - w.a > sum(M.CHAIN)     # (the longest history a kernel keeps is 160 samples)
            M.expect(cfg, iq, w)
            got = [e for _, ev in w.calls for e in ev]
            assert np.array_equal(w.history, M.decode(iq[w.a - taps:w.a])), (row.label, k, w.kind)
            assert sum(len(s) for s, _ in w.calls) in range(2 * M.WINDOW - 2, 2 * M.WINDOW + 3)
            if w.kind == "control":
                assert got == [] and w.state["locked"] == w.final["locked"], (row.label, k, got)
                continue
            assert w.event in got and w.event in w.calls[-1][1], (row.label, k, w.kind, w.event, got)
            assert w.state["locked"] == 1 - w.event[1]
            if w.kind == "lock":
                assert w.state["first_lock_symbol"] == -1 and w.final["first_lock_symbol"] == w.event[0]
            else:
                assert w.state["first_lock_symbol"] == lock[0] == w.final["first_lock_symbol"]
            at[w.kind].append(w.event[0])
    for kind in ("lock", "unlock", "relock"):
        assert len(set(at[kind])) == M.N_STREAMS, (row.label, kind, at[kind])
