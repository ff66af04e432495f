"""CPU tests of the 80 k interleaved mode (include/meteor_demod_amd_interleave.h): the host model and the tracker against the numpy
sender of interleave_util.py, built to the specification's text - the sync search over all 24 hypotheses, the tie rules against a
brute-force scorer in numpy, the gather for three branch delays, the tracker across a deleted symbol, a hypothesis change and an
inserted symbol, every refusal, and Reed-Solomon coded frames end to end through the models of the frame and transfer-frame
layers.  No GPU.  Every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import frames_util as U
import interleave_util as IU

W = IU.WINDOW


# ------------------------------------------------------------------------------------------------------------ sync search
def test_pattern_is_the_sync_word():
    from meteor_demod_amd import interleave as il
    a, b = il.model_pattern()
    assert a.tolist() == [-1, 1, -1, 1] and b.tolist() == [-1, -1, 1, 1]
    bits = [int(v > 0) for pair in zip(a, b) for v in pair]
    assert int("".join(map(str, bits)), 2) == 0x27
    assert sorted(zip(a.tolist(), b.tolist())) == [(-1, -1), (-1, 1), (1, -1), (1, 1)]      # the four constellation points


@pytest.mark.parametrize("m,want", [(0, 0), (3, 0), (4, 1), (5, 1), (2562, 1), (2563, 1), (2564, 2), (5123, 2)])
def test_window_counts(m, want):
    from meteor_demod_amd import interleave as il
    assert il.windows(m) == want
    soft = np.zeros((m, 2), dtype=np.int8)
    assert len(il.model_candidates(soft)) == want
    assert il.max_output_symbols(m) == 36 * (m // 40) + 36


def through_H(soft: np.ndarray, H: int) -> np.ndarray:
    """The stream through H = h + 8 s in int32, [m, 2]: a rail value read at index m is 0."""
    x = U.through(soft, H & 7)
    z = np.zeros(1, dtype=np.int32)
    if H >> 3 == 1:
        x = np.stack([x[:, 0], np.concatenate([x[1:, 1], z])], axis=1)
    elif H >> 3 == 2:
        x = np.stack([np.concatenate([x[1:, 0], z]), x[:, 1]], axis=1)
    return x


def brute_candidates(soft: np.ndarray):
    """The specification's sync search in numpy, independent of the model: [(position, H, score)] per window."""
    m = len(soft)
    if m < 4:
        return []
    a, b = np.array([-1, 1, -1, 1]), np.array([-1, -1, 1, 1])
    score = np.zeros((24, m - 3), dtype=np.int64)
    for H in range(24):
        x = through_H(soft, H)
        for i in range(4):
            score[H] += a[i] * x[i: m - 3 + i, 0] + b[i] * x[i: m - 3 + i, 1]
    out = []
    for w in range(-(-(m - 3) // W)):
        best = None
        for r in range(min(40, m - 3 - W * w)):
            sums = score[:, W * w + r: min(W * (w + 1), m - 3): 40].sum(axis=1)
            for H in range(24):
                if best is None or sums[H] > best[2]:
                    best = (W * w + r, H, int(sums[H]))
        out.append(best)
    return out


@pytest.mark.parametrize("esn0", [None, 3.0], ids=["clean", "3dB"])
@pytest.mark.parametrize("lead", [0, 1, 23, 39])
def test_candidates_find_phase_and_hypothesis(lead, esn0):
    """4 full windows (and what is left over) for each of the 24 H: every full window's candidate is (lead mod 40, H)."""
    from meteor_demod_amd import interleave as il
    snd = IU.random_sender(100 + lead, 4 * 64 + 7, 2, lead)
    worst = None
    for H in range(24):
        soft = snd.received(H, esn0, seed=1000 + H)
        cand = il.model_candidates(soft)
        full = (len(soft) - 3) // W
        assert full >= 4 and len(cand) == il.windows(len(soft))
        got = [(c.position - W * w, c.hypothesis) for w, c in enumerate(cand[:full])]
        assert got == [(lead, H)] * full, (H, got)
        low = min(c.score for c in cand[:full])
        worst = low if worst is None else min(worst, low)
    print(f"lead {lead}, Es/N0 {esn0}: 24 H x {full} windows found; the lowest winning score {worst} of 24576")


@pytest.mark.parametrize("kind", ["zeros", "small", "full"])
@pytest.mark.parametrize("m", [4, 45, 2563, 2564, 2 * W + 1234])
def test_model_candidates_equal_the_brute_force_scorer(m, kind):
    """The tie rules on constructed input: all zeros (every score 0: the candidate is phase 0, H 0), symbols of -1 / 0 / 1 (most
    sums tie), and the full int8 range with -128 in it (negating it gives +128 in int32)."""
    from meteor_demod_amd import interleave as il
    rng = np.random.default_rng(m)
    soft = {"zeros": np.zeros((m, 2), dtype=np.int8), "small": rng.integers(-1, 2, (m, 2)).astype(np.int8),
            "full": rng.integers(-128, 128, (m, 2)).astype(np.int8)}[kind]
    if kind == "full":
        soft[rng.integers(0, m, max(1, m // 8))] = -128
    got = [(c.position, c.hypothesis, c.score) for c in il.model_candidates(soft)]
    want = brute_candidates(soft)
    print(f"m {m} ({kind}): {got[:3]}")
    assert got == want
    if kind == "zeros":
        assert got == [(W * w, 0, 0) for w in range(len(got))]


def test_ties_go_to_the_lowest_phase_then_the_lowest_hypothesis():
    """Two sync words at phases 5 and 7 in silence tie: phase 5 stands.  A word with one rail silent ties among phases and among
    hypotheses: the lowest phase, then the lowest hypothesis stands (from the table of all 40 x 24 sums)."""
    from meteor_demod_amd import interleave as il
    a, b = il.model_pattern()
    soft = np.zeros((400, 2), dtype=np.int8)
    for p in (47, 5):
        soft[p: p + 4, 0], soft[p: p + 4, 1] = 48 * a, 48 * b
    c = il.model_candidates(soft)[0]
    assert (c.position, c.hypothesis, c.score) == (5, 0, 384) == brute_candidates(soft)[0]
    # one rail silent: hypotheses that differ only in that rail's sign or skew tie, and so do neighbouring phases under a skew
    soft = np.zeros((400, 2), dtype=np.int8)
    soft[12: 16, 0] = -48 * a
    c = il.model_candidates(soft)[0]
    table = {}
    for H in range(24):
        x = through_H(soft, H)
        for r in range(40):
            table[(r, H)] = sum(int((a * x[p: p + 4, 0] + b * x[p: p + 4, 1]).sum()) for p in range(r, 397, 40))
    top = max(table.values())
    ties = sorted(k for k, v in table.items() if v == top)
    print(f"one rail silent: candidate {c}, the (r, H) with the top score {top}: {ties}")
    assert len({r for r, _ in ties}) > 1 and sum(1 for r, _ in ties if r == ties[0][0]) > 1
    assert (c.position, c.hypothesis, c.score) == (*ties[0], top) == brute_candidates(soft)[0]


# ---------------------------------------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("M", [1, 2, 8])
def test_round_trip_returns_the_senders_bits(M):
    """Sender, sync search, tracker, gather: one segment with the sender's phase and H, P periods, every output bit whose source
    exists has the sender's hard decision, and every bit with N >= P is exactly 0."""
    from meteor_demod_amd import interleave as il
    snd = IU.random_sender(7 + M, 450, M, lead=13)
    for H in (0, 6, 9, 20, 23):
        soft = snd.received(H, None, seed=H)
        out, segs, P = il.model_decode(soft, branch_delay=M)
        assert P == 450 and [(s.first_symbol, s.marker_symbol, s.period, s.phase, s.hypothesis) for s in segs] == [(0, 13, 0, 13, H)]
        assert out.shape == (36 * P, 2)
        compared, excluded, n = IU.check_bits(snd, out, P)
        print(f"M {M}, H {H}: {compared} of {n} bits have a source and are right; the rest are 0")
        assert excluded == 0 and compared == n - sum(M * b for b in range(36)) and (np.abs(out.reshape(-1)[:n]) == 48).sum() == compared


def test_negating_minus_128_stores_127():
    from meteor_demod_amd import interleave as il
    soft = np.full((400, 2), -128, dtype=np.int8)
    for H, want in ((0, (-128, -128)), (2, (127, 127)), (4, (-128, 127)), (6, (127, -128)), (1, (127, -128)), (10, (127, 127))):
        out = il.model_deinterleave(soft, [il.Segment(0, 0, 0, 0, H)], 10, branch_delay=1)
        k = np.arange(720)
        have = (k + 36 * (k % 36)) // 72 < 10
        flat = out.reshape(-1)
        assert (flat[~have] == 0).all() and (flat[have & (k % 2 == 0)] == want[0]).all() and (flat[have & (k % 2 == 1)] == want[1]).all(), H


# ------------------------------------------------------------------------------------------------------------ the tracker
def test_tracker_follows_a_deleted_symbol_a_hypothesis_change_and_an_inserted_symbol():
    """The specification's slip stream: four segments, N0 = 0, 768, 1472, 2240, the phases 17, 16, 16, 17 and H 9, 9, 20, 20."""
    from meteor_demod_amd import interleave as il
    snd = IU.slip_sender(8)
    soft = snd.received(IU.SLIP_H[0], None, seed=3)
    segs, P = il.track(il.model_candidates(soft), len(soft))
    print(segs, P)
    assert tuple(s.period for s in segs) == IU.SLIP_PERIODS
    assert [(s.first_symbol, s.phase, s.hypothesis) for s in segs] == [(0, 17, 9), (12 * W, 16, 9), (23 * W, 16, 20), (35 * W, 17, 20)]
    assert all(s.marker_symbol == s.first_symbol + s.phase for s in segs)
    assert P == 2240 + (len(soft) - segs[-1].marker_symbol) // 40 == 3000


def test_slip_stream_bits():
    """3000 periods, the three events at least 11 windows apart, without noise: every bit whose source symbol is at least 5120
    symbols from an event is right; at most 30 % of the bits are excluded by that rule."""
    from meteor_demod_amd import interleave as il
    snd = IU.slip_sender(8)
    soft = snd.received(IU.SLIP_H[0], None, seed=3)
    out, segs, P = il.model_decode(soft, branch_delay=8)
    compared, excluded, n = IU.check_bits(snd, out, P)
    print(f"{compared} bits compared and right, {excluded} of {n} excluded ({100 * excluded / n:.1f} %)")
    assert n == 72 * 3000 and excluded / n <= 0.30


def test_no_counting_run_gives_no_segment():
    from meteor_demod_amd import frames, interleave as il
    m = 10 * W + 3
    cand = [frames.Candidate(W * w + (w % 2), 3, 100) for w in range(10)]
    assert il.track(cand, m) == ([], 0)
    assert il.track(cand, m, min_run=1)[1] > 0
    noise = U.noise(m, seed=5)
    out, segs, P = il.model_decode(noise)
    print(f"noise: {len(segs)} segments, {P} periods")
    assert (segs, P, out.shape) == ([], 0, (0, 2))
    # a run that counts, a gap of noise windows, the same (r, H) again: one segment
    cand = [frames.Candidate(W * w + 7, 5, 100) for w in range(10)]
    cand[4] = frames.Candidate(W * 4 + 30, 1, 50)
    segs, P = il.track(cand, m)
    assert len(segs) == 1 and P == (m - 7) // 40


def test_tracker_refusals():
    from meteor_demod_amd import _capi, frames, interleave as il
    m = 5 * W + 3
    good = [frames.Candidate(W * w + 7, 5, 100) for w in range(5)]
    assert il.track(good, m)[1] == (m - 7) // 40
    for name, kw, cand, mm in (("min_run 0", dict(min_run=0), good, m), ("branch_delay 0", dict(branch_delay=0), good, m),
                               ("another window", {}, good[:2] + [frames.Candidate(W * 3 + 7, 5, 100)] + good[3:], m),
                               ("phase 40", {}, good[:2] + [frames.Candidate(W * 2 + 40, 5, 100)] + good[3:], m),
                               ("past the last position", {}, good[:4] + [frames.Candidate(m - 3, 5, 100)], m),
                               ("H 24", {}, good[:2] + [frames.Candidate(W * 2 + 7, 24, 100)] + good[3:], m),
                               ("a window short", {}, good[:4], m), ("a window more", {}, good, m - W)):
        o = il.make_opts()
        for k, v in kw.items():
            setattr(o, k, v)
        segs, n, p = (il.MdemodIlSegment * 8)(), C.c_uint64(99), C.c_uint64(99)
        rc = il.lib().mdemod_il_track(C.byref(o), frames._cands_to_c(cand), len(cand), mm, segs, 8, C.byref(n), C.byref(p))
        print(f"{name}: rc {rc}, {_capi.last_error()!r}")
        assert rc == _capi.MDEMOD_ERR_PARAM and n.value == 0 and p.value == 0 and _capi.last_error(), name


def test_gather_refusals():
    from meteor_demod_amd import _capi, interleave as il
    soft = np.zeros((400, 2), dtype=np.int8)
    ok = [il.Segment(0, 3, 0, 3, 5), il.Segment(0, 203, 5, 3, 7)]
    assert il.model_deinterleave(soft, ok, 9, branch_delay=1).shape == (324, 2)
    for name, segs, P, kw in (("does not begin at period 0", [il.Segment(0, 3, 1, 3, 5)], 9, {}), ("periods descend", ok + [il.Segment(0, 243, 4, 3, 7)], 9, {}),
                              ("H 24", [il.Segment(0, 3, 0, 3, 24)], 9, {}), ("sync word past m", [il.Segment(0, 401, 0, 1, 5)], 9, {}),
                              ("periods without a segment", [], 9, {}), ("more periods than symbols", ok, 401, {}),
                              ("branch_delay 0", ok, 9, dict(branch_delay=0))):
        with pytest.raises(_capi.MdemodError) as e:
            il.model_deinterleave(soft, segs, P, **kw)
        print(f"{name}: {e.value}")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and e.value.detail, name
    assert il.model_deinterleave(soft, [], 0).shape == (0, 2)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("differential", [False, True], ids=["plain", "differential"])
@pytest.mark.parametrize("H", [0, 9, 20])
def test_rs_coded_frames_through_the_models(H, differential):
    """Four RS-coded frames, interleaved with M = 8, sent through the inverse of H at Es/N0 = 6 dB: the models of this layer, of the
    frame layer (skew off) and of the transfer-frame layer return the VCDUs that were sent, none uncorrectable, and the frame
    layer reports h = 0."""
    from meteor_demod_amd import frames, interleave as il, rs
    snd = IU.FramedSender(seed=50, M=8, n_frames=4, tail_bits=IU.tail_bits_for(8, 4, 777), differential=differential, lead=11)
    soft = snd.received(H, 6.0, seed=60 + H)
    out, segs, P = il.model_decode(soft, branch_delay=8)
    assert [(s.phase, s.hypothesis) for s in segs] == [(11, H)] and P == snd.periods
    cadu, fr = frames.model_decode(out, differential=differential)
    vcdu, info = rs.model_decode(cadu)
    rep = rs.report(vcdu, info)
    print(f"H {H}, differential {differential}: {len(soft)} symbols -> {len(out)}, {len(fr)} frames at {[f.position for f in fr]} as h "
          f"{sorted({f.hypothesis for f in fr})}, channel_errors {[f.channel_errors for f in fr]}, {rep.bytes_corrected} bytes corrected")
    assert [f.position for f in fr] == snd.positions and {f.hypothesis for f in fr} == {0}
    assert rep.uncorrectable_frames == 0 and [bytes(v) for v in vcdu] == [bytes(v) for v in snd.vcdus]
