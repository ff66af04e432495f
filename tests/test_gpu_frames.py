"""GPU tests of the frame layer (include/meteor_demod_amd_frames.h): the two kernels against the host model, byte for byte - the
marker search on random symbols, framed streams through the eight hypotheses at 7 dB (against the transmitted bytes too) and at
3 dB (where the decoder errs, and the tie rules show), the decoder alone against an independent maximum-likelihood reference
(tests/viterbi_ref.py) at 2 dB and against the model on ties, full-scale symbols and frame lists no tracker makes, the edges of a
stream, guard regions, the pieces of the host entry, a recording through the GPU demodulator and the GPU frame layer, and the C
host's --cadu.  Every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

import frames_util as U

pytestmark = pytest.mark.gpu

FRAME = 8192


def _dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{gpu_device}")


def _same(got, want):
    """(cadu, frames) of the GPU and of the model: the same frame list - channel_errors included - and the same bytes."""
    assert got[1] == want[1], (got[1], want[1])
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])


# ------------------------------------------------------------------------------------------------------------ candidates
@pytest.mark.parametrize("m,kind", [(3 * FRAME + 5000, "full"), (3 * FRAME + 5000, "ties"), (33, "full"), (FRAME + 32, "ties"), (FRAME + 33, "full"),
                                    (2 * FRAME + 31, "full")])
def test_candidates_equal_the_model(m, kind, gpu_device):
    """Random int8 over the full range, -128 included (and symbols of -1 / 0 / 1, where most scores tie): one candidate per window,
    equal to the model's in position, hypothesis and score."""
    from meteor_demod_amd import frames
    rng = np.random.default_rng(m + len(kind))
    soft = rng.integers(-128, 128, (m, 2)).astype(np.int8) if kind == "full" else rng.integers(-1, 2, (m, 2)).astype(np.int8)
    if kind == "full":
        soft[rng.integers(0, m, m // 16)] = -128
    want = frames.model_candidates(soft)
    got = frames.candidates(_dev(soft, gpu_device))
    print(f"m {m} ({kind}): {len(got)} windows, {got[:4]}")
    assert len(got) == frames.windows(m) and got == want


# --------------------------------------------------------------------------------------------------------- framed stream
@pytest.fixture(scope="module")
def stream():
    return U.Stream(seed=1)


@pytest.mark.parametrize("h", range(8))
def test_framed_stream_at_7_db(h, stream, gpu_device):
    from meteor_demod_amd import frames
    soft = stream.received(h, 7.0, seed=100 + h)
    got = frames.decode(_dev(soft, gpu_device))
    _same(got, frames.model_decode(soft))
    assert [(f.position, f.hypothesis, f.flags) for f in got[1]] == [(p, h, 0) for p in stream.positions]
    assert [bytes(c) for c in got[0]] == stream.frames
    print(f"h {h}: channel_errors {[f.channel_errors for f in got[1]]}")


@pytest.mark.parametrize("h", range(8))
def test_framed_stream_at_3_db_equals_the_model(h, stream, gpu_device):
    """At 3 dB the decoder errs and metrics tie: bytes and channel_errors still equal the model's - for the frames the tracker
    finds, and for all five decoded where they were sent."""
    from meteor_demod_amd import frames
    soft = stream.received(h, 3.0, seed=200 + h)
    d = _dev(soft, gpu_device)
    want = frames.model_decode(soft)
    _same(frames.decode(d), want)
    sent = [frames.Frame(p, h, 0, 0, 0, 0) for p in stream.positions]
    cadu, fr = frames.viterbi(d, sent)
    mc, mf = frames.model_viterbi(soft, sent)
    wrong = sum(bytes(c) != f for c, f in zip(mc, stream.frames))
    print(f"h {h}: {len(want[1])} frames tracked; decoded in place: channel_errors {[f.channel_errors for f in fr]}, {wrong} of 5 frames with byte errors")
    assert fr == mf and np.array_equal(cadu.cpu().numpy(), mc)


# ----------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("m", [0, 31, 8191])
def test_short_streams(m, gpu_device):
    import torch
    from meteor_demod_amd import frames
    soft = U.noise(m, seed=8)
    d = torch.zeros((m, 2), dtype=torch.int8, device=f"cuda:{gpu_device}")
    d.copy_(torch.from_numpy(soft))
    assert frames.candidates(d) == frames.model_candidates(soft)
    for x in (d, soft):
        cadu, fr = frames.decode(x)
        assert fr == [] and cadu.shape == (0, 1024)


def _edge_streams():
    st = U.Stream(seed=2, n_frames=4, lead=0, tail=0)
    yield "a frame at 0 and a frame ending at m", st.received(3, 7.0, seed=2), 4
    st = U.Stream(seed=3, n_frames=4, lead=100, tail=0)
    yield "the last frame one symbol short", st.received(6, 7.0, seed=3)[:-1], 3
    st = U.Stream(seed=4, n_frames=8)
    soft = st.received(5, 7.0, seed=4)
    cut = st.positions[3] + 4000
    yield "a symbol slip", np.concatenate([soft[:cut], soft[cut + 1:]]), 7
    st = U.Stream(seed=5, n_frames=8)
    h = np.zeros(len(st.sym), dtype=int)
    h[st.positions[3] + 4000:] = 1
    yield "a rotation change", st.received(h, 7.0, seed=5), 8
    st = U.Stream(seed=6, n_frames=7)
    soft = st.received(7, 7.0, seed=6)
    soft[st.positions[3]: st.positions[3] + 32] = U.noise(32, seed=60)
    yield "a lost marker", soft, 7


@pytest.mark.parametrize("case", range(5))
def test_edge_streams_equal_the_model(case, gpu_device):
    from meteor_demod_amd import frames
    name, soft, n = list(_edge_streams())[case]
    got = frames.decode(_dev(soft, gpu_device))
    print(f"{name}: {[(f.position, f.hypothesis, f.flags, f.run, f.channel_errors) for f in got[1]]}")
    assert len(got[1]) == n
    _same(got, frames.model_decode(soft))


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 16, 1001])
def test_guard_regions(shift, stream, gpu_device):
    """The input inside garbage on both sides, at a 16-byte aligned address and at an odd one: the result is that of the input
    alone.  The outputs inside guard words, the CADUs at an aligned and at an odd address: the guards stay as they were."""
    import torch
    from meteor_demod_amd import frames
    soft = stream.received(2, 7.0, seed=102)
    m = len(soft)
    rng = np.random.default_rng(shift)
    buf = rng.integers(-128, 128, 4096 + 2 * m + 4096).astype(np.int8)
    start = 2048 + shift
    buf[start: start + 2 * m] = soft.reshape(-1)
    d = _dev(buf, gpu_device)
    src = C.c_void_p(d.data_ptr() + start)
    lib, st = frames.lib(), C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    n_w = frames.windows(m)
    guard = 0x5A5A5A5A
    cand = torch.full((4 * (n_w + 2),), guard, dtype=torch.int32, device=d.device)
    rc = lib.mdemod_frames_candidates_device(src, m, C.c_void_p(cand.data_ptr() + 16), gpu_device, st)
    assert rc == 0
    c = cand.cpu().numpy().astype(np.int64)
    assert (c[:4] == guard).all() and (c[-4:] == guard).all()
    got = [frames.Candidate(int((r[0] & 0xFFFFFFFF) | (r[1] << 32)), int(r[3]), int(r[2])) for r in c[4:-4].reshape(-1, 4)]
    want = frames.model_candidates(soft)
    assert got == want
    sent = [frames.Frame(p, 2, 0, 0, 0, 0) for p in stream.positions]
    arr = frames._to_c(sent)
    pad = 64 + (shift & 1) * 3                                                # the CADUs at an aligned address, or at an odd one
    out = torch.full((pad + len(sent) * 1024 + 64,), 0xA5, dtype=torch.uint8, device=d.device)
    rc = lib.mdemod_frames_viterbi_device(src, m, arr, len(sent), C.c_void_p(out.data_ptr() + pad), gpu_device, st)
    assert rc == 0
    o = out.cpu().numpy()
    assert (o[:pad] == 0xA5).all() and (o[-64:] == 0xA5).all()
    mc, mf = frames.model_viterbi(soft, sent)
    assert np.array_equal(o[pad:-64].reshape(-1, 1024), mc) and frames._frames(arr, len(sent)) == mf
    assert [bytes(x) for x in mc] == stream.frames


# ------------------------------------------------------------------------------------------------ the decoder on its own
@pytest.mark.parametrize("h", range(8))
def test_viterbi_is_maximum_likelihood(h, gpu_device):
    """Two frames that tile a stream of 16 384 symbols at 2 dB (test_frames_host.py's streams), decoded by the kernel where they were
    sent: the bits of viterbi_ref's full-stream ML decoding, a path metric of M*, and the model's channel_errors (which are the
    header's count on the reference's bits)."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    st, soft, sym, d, best = V.ml_case(False, h, 2.0)
    sent = [frames.Frame(p, h, 0, 0, 0, 0) for p in st.positions]
    cadu, fr = frames.viterbi(_dev(soft.copy(), gpu_device), sent)
    bits = V.bits_of(cadu.cpu().numpy())
    errors, differing, metric = int((d != st.bits).sum()), int((bits != d).sum()), V.path_metric(bits, sym)
    print(f"h {h}: {errors} of {len(d)} bits of the ML decoding differ from what was sent; kernel != ML in {differing}; M* {best}, the kernel's path "
          f"{metric}; channel_errors {[f.channel_errors for f in fr]}")
    assert errors >= 10
    assert metric == best
    assert differing == 0
    assert fr == frames.model_viterbi(soft, sent)[1]
    assert [f.channel_errors for f in fr] == [V.channel_errors(d[p: p + FRAME], sym[p: p + FRAME]) for p in st.positions]


@pytest.mark.parametrize("kind", ["zeros", "ties", "full", "signal"])
def test_viterbi_on_ties_and_full_scale(kind, gpu_device):
    """8392 symbols the tracker would never call frames: all zeros (every metric ties at every step: every bit is 0), symbols of
    -1 / 0 / 1, the full int8 range with -128; eight frames through the eight hypotheses in one launch.  And a clean frame at
    +127 / -128 through the negating hypotheses 2, 3 and 7 (-128 is negated in int32): the sent bytes and 0 channel errors.  Bytes
    and channel_errors are the model's (which test_frames_host.py holds to the header's rule on these inputs)."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    if kind == "signal":
        st = U.Stream(seed=5, n_frames=1, lead=100, tail=100)
        cases = [(V.full_scale(st, h), [(100, h)]) for h in (2, 3, 7)]
    else:
        cases = [(s, a) for name, s, a in V.hostile_inputs() if name == kind]
    for soft, at in cases:
        assert len(soft) == V.HOSTILE_M
        sent = [frames.Frame(p, h, 0, 0, 0, 0) for p, h in at]
        cadu, fr = frames.viterbi(_dev(soft, gpu_device), sent)
        mc, mf = frames.model_viterbi(soft, sent)
        got = cadu.cpu().numpy()
        print(f"{kind}: {int((soft == -128).sum())} values of -128; frames (position, h) {at}: ones per frame {[int(V.bits_of(c).sum()) for c in got]}, "
              f"channel_errors {[f.channel_errors for f in fr]}")
        assert np.array_equal(got, mc) and fr == mf
        if kind == "zeros":
            assert not got.any() and all(f.channel_errors == 0 for f in fr)
        if kind == "signal":
            assert (soft == -128).any() and bytes(got[0]) == st.frames[0] and fr[0].channel_errors == 0


def _viterbi_between_canaries(d, m, sent, odd, gpu_device):
    """mdemod_frames_viterbi_device on the stream in tensor `d` into a buffer of 0xA5 - the CADUs at an aligned address, or at an odd
    one - whose first and last bytes must stay as they were: (uint8 [n, 1024], the frames with channel_errors)."""
    import torch
    from meteor_demod_amd import frames
    arr = frames._to_c(sent)
    pad = 64 + 3 * odd
    out = torch.full((pad + len(sent) * 1024 + 64,), 0xA5, dtype=torch.uint8, device=d.device)
    st = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    rc = frames.lib().mdemod_frames_viterbi_device(C.c_void_p(d.data_ptr()), m, arr, len(sent), C.c_void_p(out.data_ptr() + pad), gpu_device, st)
    assert rc == 0
    o = out.cpu().numpy()
    assert (o[:pad] == 0xA5).all() and (o[-64:] == 0xA5).all()
    return o[pad:-64].reshape(-1, 1024), frames._frames(arr, len(sent))


def test_viterbi_takes_any_frame_list(gpu_device):
    """Frame lists no tracker would make, on 2 x 8192 + 300 symbols: positions 0, 1, 127, 128, 129 (the lead-in clamped away, in part,
    and whole), 8191, m - 8192, a position twice, two frames that share one symbol, hypotheses cycling 0..7; the whole list, the list
    backwards, its first 1, 2 and 3 frames, and every frame alone; the CADUs at an aligned and at an odd address between canaries.
    Bytes and channel_errors are the model's, the canaries stay, and a frame's result does not depend on what else is in the list."""
    from meteor_demod_amd import frames
    st = U.Stream(seed=9, n_frames=2, lead=150, tail=150)
    soft = st.received(0, 3.0, seed=90)
    m = len(soft)
    assert m == 2 * FRAME + 300
    at = [0, 1, 127, 128, 129, FRAME - 1, m - FRAME, 128, 150, 150 + FRAME - 1, 0]
    sent = [frames.Frame(p, k % 8, 0, 0, 0, 0) for k, p in enumerate(at)]
    mc, mf = frames.model_viterbi(soft, sent)
    d = _dev(soft, gpu_device)
    for odd in (0, 1):
        cadu, fr = _viterbi_between_canaries(d, m, sent, odd, gpu_device)
        assert np.array_equal(cadu, mc) and fr == mf, odd
    cadu, fr = _viterbi_between_canaries(d, m, sent[::-1], 0, gpu_device)
    assert np.array_equal(cadu, mc[::-1]) and fr == mf[::-1]
    for n in (1, 2, 3):
        cadu, fr = _viterbi_between_canaries(d, m, sent[:n], n & 1, gpu_device)
        assert np.array_equal(cadu, mc[:n]) and fr == mf[:n], n
    for k, f in enumerate(sent):
        cadu, fr = _viterbi_between_canaries(d, m, [f], k & 1, gpu_device)
        assert np.array_equal(cadu[0], mc[k]) and fr == [mf[k]], k
    print(f"m {m}: {len(sent)} frames at {at}, channel_errors {[f.channel_errors for f in mf]}; the frame at 150, which is where and as one was sent, comes "
          f"back as sent: {bytes(mc[8]) == st.frames[0]}")


# ---------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("piece", [8192, 16384])
def test_host_entry_in_pieces_equals_the_device_entry(piece, gpu_device):
    """The slip stream (two runs, 65 000 symbols) through mdemod_frames_decode_host in pieces of 16 384 (and 8 192) symbols: the
    frame list and the bytes of mdemod_frames_decode_device on the whole stream."""
    from meteor_demod_amd import frames
    _, soft, n = list(_edge_streams())[2]
    whole = frames.decode(_dev(soft, gpu_device))
    parts = frames.decode(soft, piece_symbols=piece, device=gpu_device)
    assert len(whole[1]) == n
    _same(parts, whole)
    _same(frames.decode(soft, device=gpu_device), whole)                      # (one piece)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_recording_through_the_gpu_demodulator_and_the_gpu_frame_layer(gpu_device):
    """The recording of test_frames_host.py through the GPU demodulator, then the GPU frame layer: the CADUs of the frames that
    start later than one frame after the lock are the CPU path's, and the transmitted ones."""
    from meteor_demod_amd import Demodulator, frames
    st, iq = U.recording()
    cpu_soft, lock, cpu_cadu, cpu_fr = U.recording_cpu()
    with Demodulator(U.recording_cfg(), 1, gpu_device) as dm:
        soft = dm.process_host([iq])[0]
    cadu, fr = frames.decode(_dev(soft, gpu_device))
    late_cpu = [bytes(c) for c, f in zip(cpu_cadu, cpu_fr) if f.position > lock + FRAME]
    late = [bytes(c) for c, f in zip(cadu, fr) if f.position > lock + FRAME]
    print(f"{len(soft)} symbols (CPU: {len(cpu_soft)}), lock at {lock}, {len(fr)} frames, {len(late)} of them later than one frame after the lock; "
          f"soft symbols equal to the CPU's: {len(soft) == len(cpu_soft) and np.array_equal(soft, cpu_soft)}")
    assert len(late) >= 6 and late == late_cpu
    assert all(c in st.frames for c in late)


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_cadu(tmp_path, gpu_device):
    """--cadu on a small WAV: the .cadu beside the .s holds the bytes of frames.decode_file on that .s, and the line says so."""
    from conftest import ROOT
    from meteor_demod_amd import frames
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    st, iq = U.recording()
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    out = tmp_path / "pass.s"
    p = subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), "--cadu", "-o", str(out), str(wav)], capture_output=True, text=True,
                       cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    data, rep = frames.decode_file(out, device=gpu_device)
    got = (tmp_path / "pass.cadu").read_bytes()
    assert rep.frames >= 6 and len(got) == 1024 * rep.frames and got == data
    assert sum(got[k: k + 1024] in st.frames for k in range(0, len(got), 1024)) >= 6
    line = p.stdout.strip().splitlines()[-1]
    assert f"{rep.frames} frames ({rep.flywheel_frames} flywheel) in {rep.runs} runs" in line and "/ 16372" in line
    plain = subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), "-o", str(tmp_path / "plain.s"), str(wav)], capture_output=True,
                           text=True, cwd=tmp_path, timeout=300)
    assert plain.returncode == 0 and (tmp_path / "plain.s").read_bytes() == out.read_bytes() and not (tmp_path / "plain.cadu").exists()
