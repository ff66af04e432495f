"""CPU tests of the frame layer (include/meteor_demod_amd_frames.h): the code's conventions against the known marker words, the
host model (csrc/frames_host.cpp) against transmitted data it must recover, its decoder against an independent full-stream
maximum-likelihood reference (tests/viterbi_ref.py) where it errs, the tracker's cases, a recording through the CPU
demodulator and the model, the exports and guards of the new entries, the C host linked without them, and a sanitizer fuzz of the
tracker and the model.  No GPU is touched."""
from __future__ import annotations

import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import frames_util as U
from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
HEADER = ROOT / "include" / "meteor_demod_amd_frames.h"
FRAMES_SOURCES = [CSRC / "frames.hip", CSRC / "frames_host.cpp"]
FRAME = 8192


# ----------------------------------------------------------------------------------------------------- code and pattern
def test_encoded_marker_words():
    """0x1ACFFC1D from the zero state, c1 first; its complement (what LRPT decoders search for: hypothesis 2); and the two words
    with the rails swapped by a quarter turn, (not c2, c1) and (c2, not c1).  The numpy encoder and the library's agree."""
    from meteor_demod_amd import frames
    s = U.encode(np.unpackbits(np.frombuffer(U.MARKER, dtype=np.uint8)))
    assert U.word_of(s) == 0x035D49C24FF2686B
    assert U.word_of(s, invert=True) == 0xFCA2B63DB00D9794
    turned = np.stack([1 - s[:, 1], s[:, 0]], axis=1)
    assert U.word_of(turned) == 0xA9042C6B255B3E3D
    assert U.word_of(turned, invert=True) == 0x56FBD394DAA4C1C2
    sym, reg = frames.model_encode(U.MARKER)
    assert np.array_equal(sym > 0, s == 1) and reg == 0x1D                     # (the register: the last seven bits, 0011101)
    # the encoder runs on: two calls are one
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    a, r1 = frames.model_encode(data[:100])
    b, r2 = frames.model_encode(data[100:], r1)
    whole, r3 = frames.model_encode(data)
    assert np.array_equal(np.concatenate([a, b]), whole) and r2 == r3
    assert np.array_equal(whole > 0, U.encode(np.unpackbits(np.frombuffer(data, dtype=np.uint8))) == 1)


def test_pattern_is_the_low_52_bits_whatever_came_before():
    from meteor_demod_amd import frames
    a, b = frames.model_pattern()
    word = 0
    for k in range(26):
        word = (word << 2) | (int(a[k] > 0) << 1) | int(b[k] > 0)
    assert word == 0x035D49C24FF2686B & ((1 << 52) - 1)
    assert set(np.unique(a)) <= {-1, 1} and set(np.unique(b)) <= {-1, 1}
    for before in (b"\x00", b"\xff", b"\x5a", b"\x3f"):
        sym, _ = frames.model_encode(before + U.MARKER)
        assert np.array_equal(sym[8 + 6: 8 + 32, 0], a) and np.array_equal(sym[8 + 6: 8 + 32, 1], b)
    firsts = {frames.model_encode(bytes([x]) + U.MARKER)[0][8: 8 + 6].tobytes() for x in range(64)}
    assert len(firsts) > 1                                                   # the first six symbols do depend on it


# ------------------------------------------------------------------------------------------------------ synthetic stream
@pytest.fixture(scope="module")
def stream():
    return U.Stream(seed=1)


@pytest.mark.parametrize("h", range(8))
def test_model_recovers_the_stream_at_7_db(h, stream):
    """5 frames between 777 and 300 random bits at Es/N0 = 7 dB through the inverse of hypothesis h: exactly the 5 frames, at the
    right positions and h, byte for byte; channel_errors / 16372 within a factor of two of the input's hard-decision error rate."""
    from meteor_demod_amd import frames
    soft = stream.received(h, 7.0, seed=100 + h)
    cadu, fr = frames.model_decode(soft)
    assert [(f.position, f.hypothesis, f.flags) for f in fr] == [(p, h, 0) for p in stream.positions]
    assert [bytes(c) for c in cadu] == stream.frames
    assert len({f.run for f in fr}) == 1
    ber = U.hard_error_rate(soft, h, stream)
    rate = np.mean([f.channel_errors for f in fr]) / frames.FRAME_DECISIONS
    print(f"h {h}: hard-decision error rate {ber:.5f}, channel_errors / 16372 {rate:.5f}, scores {[f.score for f in fr]}")
    assert ber / 2 <= rate <= ber * 2
    cands = frames.model_candidates(soft)
    assert len(cands) == frames.windows(len(soft)) == 6
    assert [(c.position, c.hypothesis) for c in cands[:5]] == [(p, h) for p in stream.positions]


def test_minus_128_is_negated_in_int32():
    """A stream at full scale: -128 through a negating hypothesis is +128.  Scores and bytes say so."""
    from meteor_demod_amd import frames
    st = U.Stream(seed=5, n_frames=3, lead=40, tail=40)
    soft = np.where(U.through_inverse(st.sym, 2) > 0, 127, -128).astype(np.int8)
    cadu, fr = frames.model_decode(soft)
    assert [bytes(c) for c in cadu] == st.frames and all(f.hypothesis == 2 and f.channel_errors == 0 for f in fr)
    a, b = frames.model_pattern()
    want = int(np.where(a > 0, 128, 127).sum() + np.where(b > 0, 128, 127).sum())      # a coded 1: -(-128) = 128; a coded 0: -(127) times -1
    assert [f.score for f in fr] == [want] * 3


# ------------------------------------------------------------------------------------------- the decoder is maximum-likelihood
# viterbi_ref.ml_stream: two frames that tile a stream of 16 384 symbols, sent through the inverse of h with receive seed 400 + h at
# 2 dB and 500 + h at 3 dB.  Measured for these seeds (h = 0..7; bits of the full-stream ML decoding that differ from what was sent,
# of 16 384): 139 117 47 25 81 67 61 45 at 2 dB, 2 0 13 0 0 7 25 3 at 3 dB; windowed rule against full-stream decoding: 0 differing
# bits in all sixteen (no seed had to be replaced).
ML_CASES = [(h, esn0) for esn0 in (2.0, 3.0) for h in range(8)]


def _ml_errors(st, bits, esn0):
    """The premise of a 2 dB case: the ML decoder itself errs, at least 10 times over the stream."""
    errors = int((bits != st.bits).sum())
    assert esn0 != 2.0 or errors >= 10, errors
    return errors


@pytest.mark.parametrize("h,esn0", ML_CASES)
def test_reference_windowed_rule_equals_full_stream_decoding(h, esn0):
    """viterbi_ref itself: the header's sub-block rule in numpy (ml_decode on each [s - 128, s + 1152) clamped to the stream, the
    middle 1024 bits kept) gives the bits of one ml_decode over the whole stream, and those bits reach M*."""
    import viterbi_ref as V
    st, _, sym, d, best = V.ml_case(False, h, esn0)
    assert len(sym) == 2 * FRAME and st.positions == [0, FRAME]
    windowed = np.concatenate([V.windowed_decode(sym, p)[0] for p in st.positions])
    differing = int((windowed != d).sum())
    print(f"h {h}, {esn0} dB: {_ml_errors(st, d, esn0)} of {len(d)} bits of the ML decoding differ from what was sent; windowed != full-stream in "
          f"{differing}; M* {best}, metric of the decoded path {V.path_metric(d, sym)}")
    assert differing == 0
    assert V.path_metric(d, sym) == best
    assert V.path_metric(st.bits, sym) <= best                               # (what was sent is a path too)


@pytest.mark.parametrize("h,esn0", ML_CASES)
def test_model_is_maximum_likelihood(h, esn0):
    """The model's sub-block decoding of the two frames where they were sent is the full-stream ML decoding bit for bit, its path
    metric is M* (whatever the tie rules), and channel_errors is the header's count on those bits."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    st, soft, sym, d, best = V.ml_case(False, h, esn0)
    cadu, fr = frames.model_viterbi(soft, [frames.Frame(p, h, 0, 0, 0, 0) for p in st.positions])
    bits = V.bits_of(cadu)
    differing, metric = int((bits != d).sum()), V.path_metric(bits, sym)
    want_errors = [V.channel_errors(d[p: p + FRAME], sym[p: p + FRAME]) for p in st.positions]
    print(f"h {h}, {esn0} dB: {_ml_errors(st, d, esn0)} of {len(d)} bits of the ML decoding differ from what was sent; model != ML in {differing}; "
          f"M* {best}, the model's path {metric}; channel_errors {[f.channel_errors for f in fr]}")
    assert metric == best
    assert differing == 0
    assert [f.channel_errors for f in fr] == want_errors


@pytest.mark.parametrize("h", [0, 3, 6])
def test_model_is_maximum_likelihood_off_the_streams_ends(h):
    """777 bits lead and 300 trail: no window is aligned to an end of the stream.  The frames' bits are the matching slices of the
    full-stream ML decoding."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    st, soft, sym, d, best = V.ml_case(False, h, 2.0, 777, 300)
    assert st.positions == [777, 777 + FRAME] and len(sym) == 777 + 2 * FRAME + 300
    cadu, fr = frames.model_viterbi(soft, [frames.Frame(p, h, 0, 0, 0, 0) for p in st.positions])
    for c, f, p in zip(cadu, fr, st.positions):
        differing, errors = int((V.bits_of(c) != d[p: p + FRAME]).sum()), int((d[p: p + FRAME] != st.bits[p: p + FRAME]).sum())
        print(f"h {h}, frame at {p}: {errors} of {FRAME} bits of the ML decoding differ from what was sent; model != ML in {differing}; M* {best}; "
              f"channel_errors {f.channel_errors}")
        assert errors >= 10
        assert differing == 0
        assert f.channel_errors == V.channel_errors(d[p: p + FRAME], sym[p: p + FRAME])


def test_model_on_ties_and_full_scale_equals_the_windowed_rule():
    """Inputs where the tie rules decide: all zeros (every bit 0: on equal metrics the branch from s' >> 1 wins, and the lowest of
    the equal final states), symbols of -1 / 0 / 1, the full int8 range with -128.  The model's bytes and channel_errors are those of
    the header's rule in numpy (viterbi_ref.windowed_decode): on noise the windows need not merge, so the reference is the windowed
    one.  A full-scale signal through the negating hypotheses comes back as sent with 0 channel errors."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    for name, soft, at in V.hostile_inputs():
        at = [at[k] for k in (0, 3, 5, 6)]
        cadu, fr = frames.model_viterbi(soft, [frames.Frame(p, h, 0, 0, 0, 0) for p, h in at])
        for c, f, (p, h) in zip(cadu, fr, at):
            sym = V.through_H(soft, h)
            want = V.windowed_decode(sym, p)[0]
            differing = int((V.bits_of(c) != want).sum())
            print(f"{name}: frame at {p} through h {h}: {int(want.sum())} ones, model != windowed rule in {differing}, channel_errors {f.channel_errors}")
            assert differing == 0
            assert f.channel_errors == V.channel_errors(want, sym[p: p + FRAME])
            assert name != "zeros" or (not c.any() and f.channel_errors == 0)
    st = U.Stream(seed=5, n_frames=1, lead=100, tail=100)
    for h in (2, 3, 7):
        soft = V.full_scale(st, h)
        assert len(soft) == V.HOSTILE_M and (soft == -128).any()
        cadu, fr = frames.model_viterbi(soft, [frames.Frame(100, h, 0, 0, 0, 0)])
        assert bytes(cadu[0]) == st.frames[0] and fr[0].channel_errors == 0


# --------------------------------------------------------------------------------------------------------------- tracker
def _decode(soft, **opts):
    from meteor_demod_amd import frames
    return frames.model_decode(soft, **opts)


def test_tracker_min_run(stream):
    soft = stream.received(0, 7.0, seed=1)
    assert len(_decode(soft)[1]) == 5
    assert len(_decode(soft, min_run=5)[1]) == 5
    assert _decode(soft, min_run=6)[1] == []
    from meteor_demod_amd import _capi
    with pytest.raises(_capi.MdemodError) as e:
        _decode(soft, min_run=0)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "min_run" in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        _decode(soft, piece_symbols=5000)
    assert "piece_symbols" in e.value.detail
    with pytest.raises(TypeError):
        _decode(soft, minrun=3)


def test_tracker_frame_at_zero_and_frame_ending_at_m():
    st = U.Stream(seed=2, n_frames=4, lead=0, tail=0)
    soft = st.received(3, 7.0, seed=2)
    assert len(soft) == 4 * FRAME
    cadu, fr = _decode(soft)
    assert [f.position for f in fr] == [0, FRAME, 2 * FRAME, 3 * FRAME] and all(f.hypothesis == 3 for f in fr)
    assert [bytes(c) for c in cadu] == st.frames


def test_tracker_last_frame_one_symbol_short_supports_its_run():
    """4 frames, the last symbol missing: 3 frames are emitted; with min_run = 4 still 3 (the fourth candidate counts), with 5 none."""
    st = U.Stream(seed=3, n_frames=4, lead=100, tail=0)
    soft = st.received(6, 7.0, seed=3)[:-1]
    for min_run, want in ((3, 3), (4, 3), (5, 0)):
        cadu, fr = _decode(soft, min_run=min_run)
        assert [f.position for f in fr] == st.positions[:want], min_run
        assert [bytes(c) for c in cadu] == st.frames[:want]


def test_tracker_symbol_slip_gives_two_runs():
    """One symbol deleted in the middle of frame 3 of 8: the frames after it stand one symbol earlier, in a run of their own.  The
    damaged frame would overlap the next by one symbol: it yields."""
    st = U.Stream(seed=4, n_frames=8)
    soft = st.received(5, 7.0, seed=4)
    cut = st.positions[3] + 4000
    soft = np.concatenate([soft[:cut], soft[cut + 1:]])
    cadu, fr = _decode(soft)
    assert [f.position for f in fr] == st.positions[:3] + [p - 1 for p in st.positions[4:]]
    assert [f.run for f in fr] == [0] * 3 + [1] * 4 and all(f.hypothesis == 5 and not f.flywheel for f in fr)
    assert [bytes(c) for c in cadu] == st.frames[:3] + st.frames[4:]


def test_tracker_rotation_change_gives_two_runs():
    st = U.Stream(seed=5, n_frames=8)
    h = np.zeros(len(st.sym), dtype=int)
    h[st.positions[3] + 4000:] = 1
    soft = st.received(h, 7.0, seed=5)
    cadu, fr = _decode(soft)
    assert [f.position for f in fr] == st.positions
    assert [f.hypothesis for f in fr] == [0] * 4 + [1] * 4 and [f.run for f in fr] == [0] * 4 + [1] * 4
    assert [bytes(c) for k, c in enumerate(cadu) if k != 3] == [f for k, f in enumerate(st.frames) if k != 3]
    assert bytes(cadu[3])[:400] == st.frames[3][:400] and bytes(cadu[3]) != st.frames[3]


def test_tracker_flywheel_over_a_lost_marker():
    st = U.Stream(seed=6, n_frames=7)
    soft = st.received(7, 7.0, seed=6)
    p = st.positions[3]
    soft[p: p + 32] = U.noise(32, seed=60)
    cadu, fr = _decode(soft)
    assert [f.position for f in fr] == st.positions and len({f.run for f in fr}) == 1
    assert [f.flywheel for f in fr] == [False] * 3 + [True] + [False] * 3 and fr[3].score == 0 and fr[3].hypothesis == 7
    assert [bytes(c) for k, c in enumerate(cadu) if k != 3] == [f for k, f in enumerate(st.frames) if k != 3]
    assert bytes(cadu[3])[16:] == st.frames[3][16:]                           # the decoder finds its way back within a few bytes
    assert [f.flywheel for f in _decode(soft, flywheel=0)[1]] == [False] * 6   # never merged: two runs, the frame between is not emitted
    assert len(_decode(soft, flywheel=0, min_run=4)[1]) == 0


def test_tracker_noise_alone_gives_no_frame():
    soft = U.noise(64 * FRAME + 32, seed=7)
    from meteor_demod_amd import frames
    assert frames.windows(len(soft)) == 64
    assert _decode(soft)[1] == []


@pytest.mark.parametrize("m", [0, 31, 32, 8191])
def test_short_streams(m):
    from meteor_demod_amd import frames
    soft = U.noise(m, seed=8)
    assert frames.windows(m) == (1 if m > 32 else 0)
    cadu, fr = _decode(soft)
    assert fr == [] and cadu.shape == (0, 1024)
    cands = frames.model_candidates(soft)
    assert len(cands) == frames.windows(m) and all(0 <= c.position < m - 32 for c in cands)
    assert frames.track(cands, m) == []


def test_track_refuses_what_is_not_a_candidate_list():
    from meteor_demod_amd import _capi, frames
    good = [frames.Candidate(100, 0, 50), frames.Candidate(FRAME + 100, 0, 50)]
    m = 2 * FRAME + 32
    assert frames.track(good, m, min_run=2) == [frames.Frame(100, 0, 50, 0, 0, 0)]           # (the second frame is not complete)
    for bad, word in (([good[0], frames.Candidate(100, 0, 50)], "outside its window"), ([good[0], frames.Candidate(FRAME + 100, 8, 50)], "hypothesis"),
                      ([good[0]], "windows")):
        with pytest.raises(_capi.MdemodError) as e:
            frames.track(bad, m)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail


# ------------------------------------------------------------------------------------------------------------ end to end
def test_recording_through_the_cpu_demodulator_and_the_model():
    """9 frames as QPSK (RRC 0.6, 4 samples per symbol, s16, 0 Hz) through the CPU demodulator, then the host model: every frame
    that starts later than one frame after the first lock is recovered byte for byte, and there are at least 6 of them."""
    st, _ = U.recording()
    soft, lock, cadu, fr = U.recording_cpu()
    got = {bytes(c) for c in cadu}
    delay = fr[0].position - st.positions[0]                                   # the demodulator's filters: a few symbols, the same for all
    assert 0 <= delay < 64 and [f.position - delay for f in fr] == st.positions[: len(fr)]
    late = [k for k, p in enumerate(st.positions) if p + delay > lock + FRAME and p + delay + FRAME <= len(soft)]
    print(f"lock at symbol {lock}, {len(soft)} symbols, {len(fr)} frames found, {len(late)} frames later than one frame after the lock")
    assert len(late) >= 6
    for k in late:
        assert st.frames[k] in got, k
    assert all(f.channel_errors < 0.01 * 16372 for f in fr if f.position > lock + FRAME)


# ---------------------------------------------------------------------------------------------------- exports and layout
def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", HEADER.read_text(), re.M)


def test_frames_entries_exported_and_bound():
    """Every entry of the new header is exported by the library and typed in frames.py's own table; the older binding tables and
    headers are untouched; the model is exported beside them."""
    from meteor_demod_amd import _capi, frames, frontend, survey
    names = _header_entries()
    assert len(names) == 7, names
    assert all(n.startswith("mdemod_frames_") for n in names)
    lib = frames.lib()
    for n in names + list(frames.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(frames.SIGNATURES) == sorted(names)
    assert all(n.startswith("mdemod_frames_model_") for n in frames.MODEL_SIGNATURES)
    assert not any("frames" in n for n in list(_capi.SIGNATURES) + list(frontend.SIGNATURES) + list(survey.SIGNATURES))
    for h in ("meteor_demod_amd.h", "meteor_demod_amd_frontend.h", "meteor_demod_amd_survey.h"):
        assert "mdemod_frame" not in (ROOT / "include" / h).read_text()
    assert _capi.lib().mdemod_abi_version() == 5
    import meteor_demod_amd
    for n in ("frames", "Frame"):
        assert n in meteor_demod_amd.__all__ and hasattr(meteor_demod_amd, n)
    for f in ("candidates", "track", "decode", "decode_file"):
        assert callable(getattr(frames, f))


def test_frames_int_entries_are_function_try_blocks():
    """No C++ exception crosses the boundary: every int entry of the new sources is `try { MDEMOD_API_ENTER ... } MDEMOD_API_CATCH`
    (the model's entries too)."""
    from meteor_demod_amd import frames
    found = 0
    entries = set(_header_entries()) | set(frames.MODEL_SIGNATURES)
    for src in FRAMES_SOURCES:
        text = src.read_text()
        for m in re.finditer(r"^(?:extern \"C\" )?int\n(mdemod_\w+)\(", text, re.M):
            assert m.group(1) in entries, m.group(1)
            found += 1
            body = text[m.end():]
            head = body[: body.index("{")]
            assert head.rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            end = body.index("\n}")
            assert body[end:].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 5 + 3, found


def test_frames_struct_layouts(tmp_path):
    from meteor_demod_amd.frames import MdemodFrameInfo, MdemodFramesCandidate, MdemodFramesOpts
    assert C.sizeof(MdemodFramesOpts) == 16 and C.sizeof(MdemodFramesCandidate) == 16 and C.sizeof(MdemodFrameInfo) == 32
    assert MdemodFramesOpts.piece_symbols.offset == 8 and MdemodFramesCandidate.hypothesis.offset == 12
    assert MdemodFrameInfo.flags.offset == 16 and MdemodFrameInfo.channel_errors.offset == 20 and MdemodFrameInfo.run.offset == 24
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_frames.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
           'sizeof(mdemod_frames_opts), sizeof(mdemod_frames_candidate), sizeof(mdemod_frame_info), offsetof(mdemod_frame_info, channel_errors), '
           'offsetof(mdemod_frames_opts, piece_symbols)); return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 16, 32, 20, 8]


def test_frames_host_code_is_hip_free_and_kernels_use_no_atomics():
    for name in ("frames_host.cpp", "frames_host.h"):
        host = (CSRC / name).read_text()
        assert not re.search(r"\bhip[A-Z_]|__global__|__device__|hip_runtime|hip_host", host), name
    kernels = (CSRC / "frames.hip").read_text()
    code = re.sub(r"/\*.*?\*/", "", kernels, flags=re.S)
    assert "atomic" not in code.lower()
    assert "while (" not in code[: code.index("namespace {")]                # the kernels' loops are counted
    assert "__builtin_amdgcn_sdot4" in code and "__ballot" in code and "__shfl" in code


# ------------------------------------------------------------------------------------------------- the C host, no frames
def test_cli_without_frame_layer_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has no frame layer): it links, --help lists --cadu, and --cadu
    exits non-zero saying what the library lacks - not "unrecognized option" - and writes nothing.  With --stdout it is refused
    whatever the library."""
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--cadu" in h.stderr
    wav = tmp_path / "in.wav"
    wav.write_bytes(U.wav_bytes(288000, np.zeros((16384, 2), dtype=np.int16)))
    r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), "--cadu", str(wav)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0
    assert "no frame layer" in r.stderr and "unrecognized" not in r.stderr, r.stderr
    assert r.stdout == "" and sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    for exe_ in (exe, cli_exe):
        r = subprocess.run([str(exe_), "--cadu", "--stdout", str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "--stdout" in r.stderr and r.stdout == "", r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]


# ------------------------------------------------------------------------------------------------------- sanitizer fuzz
@pytest.mark.timeout(300)
def test_frames_fuzz_under_asan_ubsan(tmp_path):
    """tests/sanitize/fuzz_frames.cpp, a program of its own over frames_host.cpp: the tracker never emits a frame outside the
    stream nor two that overlap; no sanitizer report."""
    exe = tmp_path / "fuzz_frames"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                        str(ROOT / "tests" / "sanitize" / "fuzz_frames.cpp"), str(CSRC / "frames_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread",
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "3000", "7"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["cases"] == 3000 and rep["tracked"] > 1500 and rep["refused"] > 100 and rep["decoded"] > 200 and rep["frames"] > 10000, rep
