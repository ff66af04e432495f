"""CPU tests of the frame layer's link variant (include/meteor_demod_amd_frames_link.h: differential coding, a one-symbol skew
between the rails): the differential pattern against a numpy derivation, the host model (csrc/frames_host.cpp,
csrc/frames_link_host.cpp) against transmitted data it must recover through every combined hypothesis, its decoder against an
independent full-stream maximum-likelihood reference (tests/viterbi_ref.py), polarity, the edges of a stream, ties, the tracker
over (r, H), refusals, keywords, exports and layout, the C host's --diff / --skew against a stub, the
plain layer's blindness to these streams, and a sanitizer fuzz of the model and the tracker.  No GPU is touched."""
from __future__ import annotations

import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import frames_util as U
import link_util as L
from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
HEADER = ROOT / "include" / "meteor_demod_amd_frames_link.h"
LINK_SOURCES = [CSRC / "frames_link.hip", CSRC / "frames_link_host.cpp"]
FRAME = 8192
BOTH = dict(differential=True, skew=True)


# --------------------------------------------------------------------------------------------------------------- pattern
def test_differential_pattern_is_the_numpy_derivation():
    """The marker's 32 bits through NRZ-M from d[-1] = 0, encoded: symbols 6..31, whatever the encoder held before.  d[-1] = 1 gives
    the complement.  Without `differential` the pattern is the plain one."""
    from meteor_demod_amd import frames
    bits = np.unpackbits(np.frombuffer(U.MARKER, dtype=np.uint8))
    a, b = frames.model_pattern(differential=True)
    for history in (None, np.ones(6, dtype=np.uint8), np.array([1, 0, 1, 1, 0, 0], dtype=np.uint8)):
        s0 = U.encode(L.nrzm(bits, 0), history)[6:32].astype(int) * 2 - 1
        s1 = U.encode(L.nrzm(bits, 1), history)[6:32].astype(int) * 2 - 1
        assert np.array_equal(s0[:, 0], a) and np.array_equal(s0[:, 1], b)
        assert np.array_equal(s1[:, 0], -a) and np.array_equal(s1[:, 1], -b)
    pa, pb = frames.model_pattern()
    assert not (np.array_equal(a, pa) and np.array_equal(b, pb))
    assert all(np.array_equal(x, y) for x, y in zip(frames.model_pattern(differential=False), (pa, pb)))
    assert "fr_pattern_diff" in (CSRC / "frames_host.cpp").read_text()      # derived in code, from the encoder
    assert U.encode(1 - L.nrzm(bits)).tolist() == (1 - U.encode(L.nrzm(bits), np.ones(6, dtype=np.uint8))).tolist()   # encode(~d) = ~encode(d)


# ---------------------------------------------------------------------------------------------------------- switches off
def test_switches_off_is_the_plain_model():
    """The link entries with a zeroed struct and with NULL against the plain model's on the plain tests' streams, byte for byte."""
    from meteor_demod_amd import frames
    lib = frames.lib()
    off = frames.MdemodFramesLink()
    st = U.Stream(seed=1)
    for soft in (st.received(3, 7.0, seed=103), st.received(6, 3.0, seed=206), U.noise(2 * FRAME + 31, seed=8), U.noise(33, seed=8)):
        m = len(soft)
        want_c = frames.model_candidates(soft)
        want = frames.model_decode(soft)
        sent = [frames.Frame(p, 3, 0, 0, 0, 0) for p in st.positions if p + FRAME <= m]
        want_v = frames.model_viterbi(soft, sent)
        for link in (C.byref(off), None):
            assert lib.mdemod_frames_link_windows(link, m) == frames.windows(m)
            out = (frames.MdemodFramesCandidate * max(1, len(want_c)))()
            assert lib.mdemod_frames_model_link_candidates(link, soft.ctypes.data, m, out) == 0
            assert [frames.Candidate(int(c.position), int(c.hypothesis), int(c.score)) for c in out[: len(want_c)]] == want_c
            cap = max(1, m // FRAME)
            info, cadu, n = (frames.MdemodFrameInfo * cap)(), np.zeros((cap, 1024), dtype=np.uint8), C.c_uint64()
            assert lib.mdemod_frames_model_link_decode(link, None, soft.ctypes.data, m, cadu.ctypes.data, info, cap, C.byref(n)) == 0
            assert frames._frames(info, n.value) == want[1] and np.array_equal(cadu[: n.value], want[0])
            arr, cv = frames._to_c(sent), np.zeros((len(sent), 1024), dtype=np.uint8)
            assert lib.mdemod_frames_model_link_viterbi(link, soft.ctypes.data, m, arr, len(sent), cv.ctypes.data) == 0
            assert frames._frames(arr, len(sent)) == want_v[1] and np.array_equal(cv, want_v[0])
            tracked, nt = (frames.MdemodFrameInfo * cap)(), C.c_uint64()
            assert lib.mdemod_frames_link_track(link, None, frames._cands_to_c(want_c), len(want_c), m, tracked, cap, C.byref(nt)) == 0
            assert frames._frames(tracked, nt.value) == frames.track(want_c, m)
    # the keywords at their defaults go to the plain entries
    soft = st.received(3, 7.0, seed=103)
    assert frames.model_decode(soft, differential=False, skew=False)[1] == frames.model_decode(soft)[1]


# ------------------------------------------------------------------------------------------------------ synthetic stream
@pytest.fixture(scope="module")
def streams():
    return {False: L.LinkStream(seed=1), True: L.LinkStream(seed=1, differential=True)}


@pytest.mark.parametrize("differential,H", [(False, H) for H in L.PLAIN_H] + [(True, H) for H in L.DIFF_H + [2, 11, 22]])
def test_model_recovers_the_stream_at_7_db(differential, H, streams):
    """5 frames between 777 and 300 random bits at Es/N0 = 7 dB through the inverse of the combined hypothesis H: exactly the 5
    frames, at the right positions, with that H (under `differential` its partner with h in {0, 1, 4, 5}), byte for byte."""
    from meteor_demod_amd import frames
    st = streams[differential]
    soft = st.received(H, 7.0, seed=100 + H)
    cadu, fr = frames.model_decode(soft, differential=differential, skew=True)
    want_h = L.canonical(H, differential)
    print(f"H {H} (differential {differential}): found as {[f.hypothesis for f in fr]}, scores {[f.score for f in fr]}, channel_errors {[f.channel_errors for f in fr]}")
    assert [(f.position, f.hypothesis, f.flags) for f in fr] == [(p, want_h, 0) for p in st.positions]
    assert [bytes(c) for c in cadu] == st.frames
    assert len({f.run for f in fr}) == 1 and all(f.score > 0 for f in fr)
    ber = float(((L.skew_inverse(st.sym, H) > 0) != (U.AMP * soft.astype(np.float64) > 0)).mean())
    rate = np.mean([f.channel_errors for f in fr]) / frames.FRAME_DECISIONS
    assert ber / 2 <= rate <= ber * 2, (ber, rate)                            # counted on d: the input's hard-decision error rate
    cands = frames.model_candidates(soft, differential=differential, skew=True)
    assert len(cands) == frames.windows(len(soft), skew=True) == 6
    assert [(c.position, c.hypothesis) for c in cands[:5]] == [(p, want_h) for p in st.positions]


def test_the_plain_layer_finds_none_of_it(streams):
    """The gap on record: the plain frames.decode's model on a differential stream, on a skewed one and on both finds no frame,
    or bytes that were not sent."""
    from meteor_demod_amd import frames
    for differential, H in ((True, 0), (False, 9), (False, 20), (True, 9), (True, 16)):
        st = streams[differential]
        soft = st.received(H, 7.0, seed=100 + H)
        cadu, fr = frames.model_decode(soft)
        right = sum(bytes(c) in st.frames for c in cadu)
        print(f"differential {differential}, H {H}: the plain layer finds {len(fr)} frames, {right} of them as sent")
        assert right == 0
        assert [bytes(c) for c in frames.model_decode(soft, differential=differential, skew=True)[0]] == st.frames


# ------------------------------------------------------------------------------------------- the decoder is maximum-likelihood
# viterbi_ref.ml_stream through the link sender: two frames that tile a stream of 16 384 symbols, sent through the inverse of H with
# receive seed 400 + H at 2 dB and 500 + H at 3 dB.  s = 0, 1, 2 with h swapped and not, both modes; under `differential` H = 2 and 15
# are sent upside down and decoded as their partners 0 and 13.  Measured for these seeds (bits of the full-stream ML decoding, NRZ-M
# undone, that differ from what was sent, of 16 384): plain coding H 3: 25, 9: 89, 12: 102, 18: 52, 21: 140; differential H 0: 133,
# 5: 78, 9: 134, 12: 63, 16: 102, 21: 105, 2: 83, 15: 43 at 2 dB; 12 (H 9) and 12 (differential, H 16) at 3 dB; windowed rule against
# full-stream decoding: 0 differing bits in all fifteen (no seed had to be replaced).
LINK_ML_CASES = ([(False, H, 2.0) for H in (3, 9, 12, 18, 21)] + [(True, H, 2.0) for H in (0, 5, 9, 12, 16, 21, 2, 15)]
                 + [(False, 9, 3.0), (True, 16, 3.0)])


def _ml_errors(st, bits, esn0):
    """The premise of a 2 dB case: the ML decoder itself errs, at least 10 times over the stream."""
    errors = int((bits != st.bits).sum())
    assert esn0 != 2.0 or errors >= 10, errors
    return errors


@pytest.mark.parametrize("differential,H,esn0", LINK_ML_CASES)
def test_reference_windowed_rule_equals_full_stream_decoding(differential, H, esn0):
    """viterbi_ref itself, on the link streams: the header's sub-block rule in numpy - with `differential` the xor with the bit before
    taken inside each sub-block's own decoding - gives the bits of one decoding of the whole stream."""
    import viterbi_ref as V
    st, _, sym, d, best = V.ml_case(differential, H, esn0)
    want = V.nrzm_undo(d) if differential else d
    parts = [V.windowed_decode(sym, p, differential) for p in st.positions]
    differing = int((np.concatenate([b for b, _ in parts]) != want).sum()), int((np.concatenate([own for _, own in parts]) != d).sum())
    print(f"H {H} (differential {differential}), {esn0} dB: {_ml_errors(st, want, esn0)} of {len(d)} bits of the ML decoding differ from what was sent; "
          f"windowed != full-stream in {differing[0]} (the decoder's own bits: {differing[1]}); M* {best}")
    assert differing == (0, 0)
    assert V.path_metric(d, sym) == best


@pytest.mark.parametrize("differential,H,esn0", LINK_ML_CASES)
def test_model_is_maximum_likelihood(differential, H, esn0):
    """The model's CADU bits of the two frames where they were sent are the full-stream ML decoding (NRZ-M undone under
    `differential`) bit for bit; the decoder's own bits d - the model's output coded again from the 0 that stands before step 0 -
    reach M*; and channel_errors is the header's count on d."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    st, soft, sym, d, best = V.ml_case(differential, H, esn0)
    want = V.nrzm_undo(d) if differential else d
    Hc = L.canonical(H, differential)
    cadu, fr = frames.model_viterbi(soft, [frames.Frame(p, Hc, 0, 0, 0, 0) for p in st.positions], differential=differential, skew=True)
    bits = V.bits_of(cadu)
    own = L.nrzm(bits) if differential else bits
    differing, metric = int((bits != want).sum()), V.path_metric(own, sym)
    print(f"H {H} as {Hc} (differential {differential}), {esn0} dB: {_ml_errors(st, want, esn0)} of {len(d)} bits of the ML decoding differ from what was "
          f"sent; model != ML in {differing}; M* {best}, the model's path {metric}; channel_errors {[f.channel_errors for f in fr]}")
    assert metric == best
    assert differing == 0
    assert [f.channel_errors for f in fr] == [V.channel_errors(d[p: p + FRAME], sym[p: p + FRAME]) for p in st.positions]


def test_model_on_ties_and_full_scale_equals_the_windowed_rule():
    """All zeros, symbols of -1 / 0 / 1 and the full int8 range with -128 through combined hypotheses of every skew, with and
    without `differential`: the model's bytes and channel_errors are those of the header's rule in numpy.  Frames at 0 (no bit
    before step 0) and at m - 8192 (the late rail is read at index m) are among them."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    for differential, hyps in ((True, (9, 16, 5, 20)), (False, (18, 11, 7, 12))):
        for name, soft, at in V.hostile_inputs():
            at = [(at[i][0], H) for i, H in zip((0, 7, 3, 5), hyps)]
            assert [p for p, _ in at][:2] == [0, len(soft) - FRAME]
            cadu, fr = frames.model_viterbi(soft, [frames.Frame(p, H, 0, 0, 0, 0) for p, H in at], differential=differential, skew=True)
            for c, f, (p, H) in zip(cadu, fr, at):
                sym = V.through_H(soft, H)
                want, own = V.windowed_decode(sym, p, differential)
                differing = int((V.bits_of(c) != want).sum())
                print(f"{name} (differential {differential}): frame at {p} through H {H}: {int(want.sum())} ones, model != windowed rule in {differing}, "
                      f"channel_errors {f.channel_errors}")
                assert differing == 0
                assert f.channel_errors == V.channel_errors(own, sym[p: p + FRAME])
                assert name != "zeros" or (not c.any() and f.channel_errors == 0)
    st = L.LinkStream(seed=5, n_frames=1, lead=100, tail=100, differential=True)
    for H in (1 + 8, 4 + 16, 2 + 8):                                           # h = 1 and 4 negate a rail: -128 is read as +128; 10 is sent upside down and read through 8
        soft = V.full_scale(st, H)
        assert len(soft) == V.HOSTILE_M and (soft == -128).any()
        cadu, fr = frames.model_viterbi(soft, [frames.Frame(100, L.canonical(H, True), 0, 0, 0, 0)], differential=True, skew=True)
        assert bytes(cadu[0]) == st.frames[0] and fr[0].channel_errors == 0


# -------------------------------------------------------------------------------------------------------------- polarity
def test_both_polarities_decode_to_the_same_bytes():
    """The same frames from d[-1] = 0 and d[-1] = 1, and received upside down: the same CADUs, the same hypothesis."""
    from meteor_demod_amd import frames
    a, b = L.LinkStream(seed=3, differential=True, before=0), L.LinkStream(seed=3, differential=True, before=1)
    assert a.frames == b.frames and np.array_equal(a.sym[6:], -b.sym[6:])        # (the encoder began from the zero state in both)
    results = []
    for st, H in ((a, 5), (b, 5), (a, 7), (a, 13), (b, 13), (a, 15)):
        cadu, fr = frames.model_decode(st.received(H, 7.0, seed=30), **BOTH)
        results.append(([bytes(c) for c in cadu], [(f.position, f.hypothesis) for f in fr]))
        assert results[-1][0] == st.frames and [h for _, h in results[-1][1]] == [L.canonical(H, True)] * 5
    assert results[0] == results[1] == results[2] and results[3] == results[4] == results[5]


def test_polarity_flip_in_mid_stream_costs_one_frame():
    """The polarity turns over in the middle of frame 3 of 8, as a PLL's 180 degree slip does: one run, all 8 frames found, and
    only the frame the flip lands in has wrong bytes (around the flip)."""
    from meteor_demod_amd import frames
    st = L.LinkStream(seed=4, n_frames=8, differential=True)
    sign = np.ones(len(st.sym))
    sign[st.positions[3] + 4000:] = -1
    for H in (0, 13):
        cadu, fr = frames.model_decode(st.received(H, 7.0, seed=40, sign=sign), **BOTH)
        assert [(f.position, f.hypothesis, f.run) for f in fr] == [(p, H, 0) for p in st.positions]
        assert [bytes(c) for k, c in enumerate(cadu) if k != 3] == [f for k, f in enumerate(st.frames) if k != 3]
        hit = np.flatnonzero(np.frombuffer(bytes(cadu[3]), dtype=np.uint8) != np.frombuffer(st.frames[3], dtype=np.uint8))
        print(f"H {H}: bytes of frame 3 that differ: {hit.tolist()}")
        assert len(hit) <= 4 and all(495 <= x <= 505 for x in hit)           # (bit 4000 is in byte 500)


# ----------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("m", [0, 32, 33, 34, FRAME + 33, FRAME + 34])
def test_short_streams(m):
    from meteor_demod_amd import frames
    soft = U.noise(m, seed=8)
    want = 0 if m <= 33 else (1 if m <= FRAME + 33 else 2)
    assert frames.windows(m, skew=True) == want and frames.windows(m) == (m - 32 + FRAME - 1) // FRAME * (m > 32)
    for sw in (dict(skew=True), BOTH):
        cadu, fr = frames.model_decode(soft, **sw)
        assert fr == [] and cadu.shape == (0, 1024)
        cands = frames.model_candidates(soft, **sw)
        assert len(cands) == want and all(0 <= c.position < m - 33 and c.position // FRAME == w for w, c in enumerate(cands))
        assert frames.track(cands, m, **sw) == []
    cands = frames.model_candidates(soft, differential=True)                   # without skew: the plain layer's positions
    assert len(cands) == frames.windows(m) and all(c.position < m - 32 and c.hypothesis in (0, 1, 4, 5) and c.score >= 0 for c in cands)


def test_frame_at_zero_and_frame_ending_at_m():
    """4 frames and nothing else.  The frame at 0 has no lead-in: the bit before its first is 0, which is what the sender's d[-1]
    was.  Under s = 1 and s = 2 the last frame's late rail ends one past the stream: it is read as 0, and the frame is still
    decoded (the last bits lean on one rail)."""
    from meteor_demod_amd import frames
    st = L.LinkStream(seed=2, n_frames=4, lead=0, tail=0, differential=True)
    for H in (4, 9, 20):
        soft = st.received(H, 7.0, seed=2)
        assert len(soft) == 4 * FRAME
        cadu, fr = frames.model_decode(soft, **BOTH)
        assert [(f.position, f.hypothesis) for f in fr] == [(FRAME * k, H) for k in range(4)]
        assert [bytes(c) for c in cadu[:3]] == st.frames[:3]
        assert bytes(cadu[3])[:1020] == st.frames[3][:1020]                   # (the truncated end may cost the last bits)
    # previous bit 0 at position 0: a sender that began from d[-1] = 1 is read with its first bit turned over, and only that one
    st1 = L.LinkStream(seed=2, n_frames=4, lead=0, tail=0, differential=True, before=1)
    cadu, fr = frames.model_decode(st1.received(4, None, seed=0), **BOTH)
    assert bytes(cadu[0])[0] == st1.frames[0][0] ^ 0x80 and bytes(cadu[0])[1:] == st1.frames[0][1:] and bytes(cadu[1]) == st1.frames[1]
    # the zero past the end, exactly: a clean stream whose late rail is cut decodes as the same stream with a 0 appended
    for H in (9, 20):
        soft = st.received(H, None, seed=0)
        longer = np.concatenate([soft, np.zeros((1, 2), dtype=np.int8)])
        sent = [frames.Frame(3 * FRAME, H, 0, 0, 0, 0)]
        a, b = frames.model_viterbi(soft, sent, **BOTH), frames.model_viterbi(longer, sent, **BOTH)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_ties_go_to_the_lowest_position_then_the_lowest_hypothesis():
    """A constant stream: every position ties.  The first position wins, and the lowest H among the equal best scores."""
    from meteor_demod_amd import frames
    m = FRAME + 500
    for value in ((5, 5), (0, 0), (-3, 7)):
        soft = np.tile(np.array(value, dtype=np.int8), (m, 1))
        for sw in (dict(differential=True), dict(skew=True), BOTH):
            a, b = frames.model_pattern(differential=sw.get("differential", False))
            allowed = [H for H in range(24 if sw.get("skew") else 8) if not (sw.get("differential") and H & 2)]
            scores = {}
            for H in allowed:
                x = U.through(soft[:40].astype(np.int32), H & 7)
                s = int((x[:26, 0] * a).sum() + (x[:26, 1] * b).sum())        # constant rails: a skew changes nothing
                scores[H] = abs(s) if sw.get("differential") else s
            best = max(scores.values())
            want_h = min(H for H in allowed if scores[H] == best)
            cands = frames.model_candidates(soft, **sw)
            assert [(c.position, c.hypothesis, c.score) for c in cands] == [(0, want_h, best), (FRAME, want_h, best)], (value, sw)


# --------------------------------------------------------------------------------------------------------------- tracker
def test_tracker_skew_change_gives_two_runs():
    from meteor_demod_amd import frames
    st = L.LinkStream(seed=5, n_frames=8, differential=True)
    cut = st.positions[3] + 4000
    soft = np.concatenate([st.received(0, 7.0, seed=5)[:cut], st.received(8, 7.0, seed=5)[cut:]])
    cadu, fr = frames.model_decode(soft, **BOTH)
    assert [f.position for f in fr] == st.positions
    assert [f.hypothesis for f in fr] == [0] * 4 + [8] * 4 and [f.run for f in fr] == [0] * 4 + [1] * 4
    assert [bytes(c) for k, c in enumerate(cadu) if k != 3] == [f for k, f in enumerate(st.frames) if k != 3]
    cands = frames.model_candidates(soft, **BOTH)
    assert frames.track(cands, len(soft), **BOTH) == [frames.Frame(f.position, f.hypothesis, f.score, f.flags, 0, f.run) for f in fr]


def test_refusals():
    from meteor_demod_amd import _capi, frames
    m = 2 * FRAME + 33
    good = [frames.Candidate(100, 9, 50), frames.Candidate(FRAME + 100, 9, 50)]
    assert frames.track(good, m, min_run=2, skew=True) == [frames.Frame(100, 9, 50, 0, 0, 0)]
    assert frames.track([frames.Candidate(100, 21, 50), frames.Candidate(FRAME + 100, 21, 50)], m, min_run=2, **BOTH)[0].hypothesis == 21
    m0 = 2 * FRAME + 32                                                        # without skew: two windows as well
    cases = [(dict(skew=True), m, [good[0], frames.Candidate(FRAME + 100, 24, 50)], "hypothesis"),
             (dict(differential=True), m0, [good[0], good[1]], "hypothesis"),                   # H = 9 needs skew
             (BOTH, m, [good[0], frames.Candidate(FRAME + 100, 10, 50)], "differential set"),
             (dict(differential=True), m0, [frames.Candidate(100, 2, 50), frames.Candidate(FRAME + 100, 2, 50)], "differential set"),
             (dict(skew=True), m, [good[0]], "windows"),
             (dict(differential=True), m, [good[0], good[1]], "windows"),                       # three windows without skew
             (dict(skew=True), m, [good[0], frames.Candidate(2 * FRAME - 1, 9, 50)], None)]
    for sw, mm, cands, word in cases:
        if word is None:                                                       # position m - 34 is the last one with skew: accepted
            assert frames.track(cands, mm, **sw) == []
            continue
        with pytest.raises(_capi.MdemodError) as e:
            frames.track(cands, mm, **sw)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail
    with pytest.raises(_capi.MdemodError) as e:                                # one symbol more: a third window with skew as well
        frames.track(good, 2 * FRAME + 34, skew=True)
    assert "windows" in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        frames.track([good[0], frames.Candidate(2 * FRAME, 9, 50)], m, skew=True)
    assert "outside its window" in e.value.detail
    soft = U.noise(m, seed=1)
    for sw, H, word in ((dict(skew=True), 24, "hypothesis"), (BOTH, 18, "differential set"), (dict(differential=True), 8, "hypothesis"),
                        (dict(differential=True), 3, "differential set")):
        with pytest.raises(_capi.MdemodError) as e:
            frames.model_viterbi(soft, [frames.Frame(0, H, 0, 0, 0, 0)], **sw)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        frames.model_viterbi(soft, [frames.Frame(FRAME + 34, 9, 0, 0, 0, 0)], skew=True)
    assert "not complete" in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:                                # the plain entries keep refusing H above 7
        frames.model_viterbi(soft, [frames.Frame(0, 8, 0, 0, 0, 0)])
    assert "hypothesis" in e.value.detail
    lib = frames.lib()
    bad = frames.MdemodFramesLink()
    bad.skew = 2
    n = C.c_uint64()
    assert lib.mdemod_frames_model_link_decode(C.byref(bad), None, soft.ctypes.data, m, None, None, 0, C.byref(n)) == _capi.MDEMOD_ERR_PARAM
    bad.skew, bad.reserved[1] = 1, 7
    assert lib.mdemod_frames_model_link_decode(C.byref(bad), None, soft.ctypes.data, m, None, None, 0, C.byref(n)) == _capi.MDEMOD_ERR_PARAM
    assert "reserved" in _capi.lib().mdemod_last_error().decode()


def test_python_keyword_errors():
    from meteor_demod_amd import frames
    soft = U.noise(100, seed=1)
    for call in (lambda: frames.model_decode(soft, skew=1), lambda: frames.model_candidates(soft, differential="yes"),
                 lambda: frames.track([], 10, skew=None), lambda: frames.model_viterbi(soft, [], differential=0)):
        with pytest.raises(TypeError) as e:
            call()
        assert "switch" in str(e.value)
    with pytest.raises(TypeError):
        frames.model_decode(soft, skewed=True)
    with pytest.raises(TypeError):
        frames.model_candidates(soft, True)                                    # keywords only
    assert frames.make_link() is None and frames.make_link(np.bool_(True), False).differential == 1


# ---------------------------------------------------------------------------------------------------- exports and layout
def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", HEADER.read_text(), re.M)


def test_link_entries_exported_and_bound():
    from meteor_demod_amd import _capi, frames
    names = _header_entries()
    assert sorted(names) == sorted(frames.LINK_SIGNATURES) and len(names) == 6
    assert {n.replace("_link", "") for n in names} <= set(frames.SIGNATURES)   # parallel to the plain entries
    lib = frames.lib()
    for n in names + list(frames.LINK_MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert all(n.startswith("mdemod_frames_model_link_") for n in frames.LINK_MODEL_SIGNATURES)
    assert _capi.lib().mdemod_abi_version() == 5
    import inspect
    for f in ("candidates", "track", "viterbi", "model_candidates", "model_viterbi"):
        assert {"differential", "skew"} <= set(inspect.signature(getattr(frames, f)).parameters), f


def test_link_int_entries_are_function_try_blocks():
    from meteor_demod_amd import frames
    found = 0
    entries = set(_header_entries()) | set(frames.LINK_MODEL_SIGNATURES)
    for src in LINK_SOURCES:
        text = src.read_text()
        for m in re.finditer(r"^int\n(mdemod_\w+)\(", text, re.M):
            assert m.group(1) in entries, m.group(1)
            found += 1
            body = text[m.end():]
            assert body[: body.index("{")].rstrip().endswith("try"), m.group(1)
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            assert body[body.index("\n}"):].startswith("\n} MDEMOD_API_CATCH"), m.group(1)
    assert found == 4 + 4, found
    host = (CSRC / "frames_link_host.cpp").read_text()
    assert not re.search(r"\bhip[A-Z_]|__global__|__device__|hip_runtime|hip_host", host)
    assert "fr_track(" in host and "fr_track(" in (CSRC / "frames.hip").read_text()          # one tracker, shared
    assert len(re.findall(r"^fr_track\(", "".join(p.read_text() for p in CSRC.glob("frames*")), re.M)) == 1


def test_link_struct_layout(tmp_path):
    from meteor_demod_amd.frames import MdemodFramesLink
    assert C.sizeof(MdemodFramesLink) == 16 and MdemodFramesLink.skew.offset == 4 and MdemodFramesLink.reserved.offset == 8
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_frames_link.h"\nint main(void){printf("%zu %zu %zu %zu\\n", '
           'sizeof(mdemod_frames_link), offsetof(mdemod_frames_link, skew), offsetof(mdemod_frames_link, reserved), sizeof(mdemod_frame_info)); return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 4, 8, 32]


# ------------------------------------------------------------------------------------------------------------ the C host
def test_cli_flags_against_the_stub(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (no frame layer): it links, --help names the flags and the N2-3 / N2-4
    recipe; --diff / --skew without --cadu / --vcdu are refused with a sentence; with --cadu the missing frame layer is named.
    Against a stub that has the plain frame layer only, the missing link variant is named.  Nothing is written."""
    wav = tmp_path / "in.wav"
    wav.write_bytes(U.wav_bytes(288000, np.zeros((16384, 2), dtype=np.int16)))
    plain = tmp_path / "plain_frames.c"
    plain.write_text('#include "meteor_demod_amd_frames.h"\nvoid mdemod_frames_default_opts(mdemod_frames_opts *o) { (void)o; }\n'
                     'int mdemod_frames_decode_host(const mdemod_frames_opts *o, const int8_t *s, uint64_t m, uint8_t *c, mdemod_frame_info *f, uint64_t cap, '
                     'uint64_t *n, int d) { (void)o; (void)s; (void)m; (void)c; (void)f; (void)cap; (void)d; *n = 0; return 0; }\n')
    exes = {}
    for name, extra in (("cli_stub", []), ("cli_plain", [str(plain)])):
        exes[name] = tmp_path / name
        r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                            str(ROOT / "tests" / "sanitize" / "stub_backend.c"), *extra, "-pthread", "-lm", "-o", str(exes[name])], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    before = sorted(p.name for p in tmp_path.iterdir())
    h = subprocess.run([str(exes["cli_stub"]), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--diff" in h.stderr and "--skew" in h.stderr and "-m oqpsk --skew --diff" in h.stderr and "N2-3" in h.stderr
    run = lambda exe, *flags: subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), *flags, str(wav)], capture_output=True, text=True, cwd=tmp_path)   # noqa: E731
    for exe in exes.values():
        for flags in (("--diff",), ("--skew",), ("-m", "oqpsk", "--skew", "--diff")):
            r = run(exe, *flags)
            assert r.returncode == 1 and "only with --cadu or --vcdu" in r.stderr and "unrecognized" not in r.stderr and r.stdout == "", r.stderr
    r = run(exes["cli_stub"], "--cadu", "--diff")
    assert r.returncode == 1 and "no frame layer" in r.stderr
    for flags in (("--cadu", "--diff"), ("--cadu", "--skew")):
        r = run(exes["cli_plain"], *flags)
        assert r.returncode == 1 and "no link variant" in r.stderr and "unrecognized" not in r.stderr, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == before


# ------------------------------------------------------------------------------------------------------- sanitizer fuzz
@pytest.mark.timeout(300)
def test_frames_link_fuzz_under_asan_ubsan(tmp_path):
    """tests/sanitize/fuzz_frames_link.cpp, a program of its own over frames_host.cpp and frames_link_host.cpp: the link tracker and
    the link model over random modes, candidate lists and short streams; no sanitizer report."""
    exe = tmp_path / "fuzz_frames_link"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                        str(ROOT / "tests" / "sanitize" / "fuzz_frames_link.cpp"), str(CSRC / "frames_host.cpp"), str(CSRC / "frames_link_host.cpp"),
                        str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "1500", "7"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["cases"] == 1500 and rep["tracked"] > 700 and rep["refused"] > 50 and rep["decoded"] > 100 and rep["frames"] > 3000, rep
