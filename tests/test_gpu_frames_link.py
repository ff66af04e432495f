"""GPU tests of the frame layer's link variant (include/meteor_demod_amd_frames_link.h): the link instances of the kernels against
the host model, byte for byte - the marker search over all H on random symbols and at the edges of a stream, framed streams through
every combined hypothesis at 3 dB, the decoder alone against an independent maximum-likelihood reference (tests/viterbi_ref.py) at
2 dB and against the model on ties, full-scale symbols, frame lists no tracker makes and the two ends of a stream, guard regions (the reads at index m), the pieces of the host entry (one symbol longer under
skew), the link entries with both switches off against the plain ones, an NRZ-M OQPSK recording through the GPU demodulator and the
GPU frame layer at four carrier phases, and the C host's --skew --diff.  Every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

import frames_util as U
import link_util as L

pytestmark = pytest.mark.gpu

FRAME = 8192
SWITCHES = [dict(differential=True, skew=False), dict(differential=False, skew=True), dict(differential=True, skew=True)]


def _dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{gpu_device}")


def _same(got, want):
    """(cadu, frames) of the GPU and of the model: the same frame list - channel_errors included - and the same bytes."""
    assert got[1] == want[1], (got[1], want[1])
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])


def _name(sw):
    return ("diff" if sw["differential"] else "") + ("+" if sw["differential"] and sw["skew"] else "") + ("skew" if sw["skew"] else "")


# ------------------------------------------------------------------------------------------------------------ candidates
@pytest.mark.parametrize("sw", SWITCHES, ids=_name)
@pytest.mark.parametrize("kind", ["full", "ties"])
@pytest.mark.parametrize("m", [33, 34, FRAME + 33, FRAME + 34, 3 * FRAME + 5000])
def test_candidates_equal_the_model(m, kind, sw, gpu_device):
    """Random int8 over the full range, -128 included (and symbols of -1 / 0 / 1, where most scores tie): one candidate per window,
    equal to the model's in position, combined hypothesis and score."""
    from meteor_demod_amd import frames
    rng = np.random.default_rng(m + len(kind))
    soft = rng.integers(-128, 128, (m, 2)).astype(np.int8) if kind == "full" else rng.integers(-1, 2, (m, 2)).astype(np.int8)
    if kind == "full":
        soft[rng.integers(0, m, m // 16)] = -128
    want = frames.model_candidates(soft, **sw)
    got = frames.candidates(_dev(soft, gpu_device), **sw)
    print(f"m {m} ({kind}, {_name(sw)}): {len(got)} windows, {got[:4]}")
    assert len(got) == frames.windows(m, skew=sw["skew"]) == len(want) and got == want


# --------------------------------------------------------------------------------------------------------- framed stream
@pytest.fixture(scope="module")
def streams():
    return {False: L.LinkStream(seed=1), True: L.LinkStream(seed=1, differential=True)}


@pytest.mark.parametrize("differential,H", [(False, H) for H in L.PLAIN_H] + [(True, H) for H in L.DIFF_H])
def test_framed_stream_at_3_db_equals_the_model(differential, H, streams, gpu_device):
    """5 frames at 3 dB through the inverse of H (where the decoder errs and metrics tie): candidates, frames, CADUs and
    channel_errors equal the model's - for what the tracker finds, and for all five frames decoded where they were sent."""
    from meteor_demod_amd import frames
    st = streams[differential]
    sw = dict(differential=differential, skew=True)
    soft = st.received(H, 3.0, seed=300 + H)
    d = _dev(soft, gpu_device)
    assert frames.candidates(d, **sw) == frames.model_candidates(soft, **sw)
    want = frames.model_decode(soft, **sw)
    _same(frames.decode(d, **sw), want)
    sent = [frames.Frame(p, L.canonical(H, differential), 0, 0, 0, 0) for p in st.positions]
    cadu, fr = frames.viterbi(d, sent, **sw)
    mc, mf = frames.model_viterbi(soft, sent, **sw)
    wrong = sum(bytes(c) != f for c, f in zip(mc, st.frames))
    print(f"H {H} ({_name(sw)}): {len(want[1])} frames tracked as {sorted({f.hypothesis for f in want[1]})}; decoded in place: channel_errors "
          f"{[f.channel_errors for f in fr]}, {wrong} of 5 frames with byte errors")
    assert fr == mf and np.array_equal(cadu.cpu().numpy(), mc)


# ----------------------------------------------------------------------------------------------------------------- edges
def _edge_streams():
    st = L.LinkStream(seed=2, n_frames=4, lead=0, tail=0, differential=True)
    yield "a frame at 0 (previous bit 0) and a frame ending at m, s = 1", st.received(9, 7.0, seed=2), 4
    yield "a frame at 0 and a frame ending at m, s = 2", st.received(20, 7.0, seed=3), 4
    st = L.LinkStream(seed=4, n_frames=8, differential=True)
    soft = np.concatenate([st.received(0, 7.0, seed=4)[: st.positions[3] + 4000], st.received(8, 7.0, seed=4)[st.positions[3] + 4000:]])
    yield "a skew change", soft, 8
    sign = np.ones(len(st.sym))
    sign[st.positions[3] + 4000:] = -1
    yield "a polarity flip in mid-stream", st.received(13, 7.0, seed=5, sign=sign), 8


@pytest.mark.parametrize("case", range(4))
def test_edge_streams_equal_the_model(case, gpu_device):
    from meteor_demod_amd import frames
    name, soft, n = list(_edge_streams())[case]
    sw = dict(differential=True, skew=True)
    got = frames.decode(_dev(soft, gpu_device), **sw)
    print(f"{name}: {[(f.position, f.hypothesis, f.flags, f.run, f.channel_errors) for f in got[1]]}")
    assert len(got[1]) == n
    _same(got, frames.model_decode(soft, **sw))


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 16, 1001])
def test_guard_regions(shift, gpu_device):
    """The input inside canaries of +-127 on both sides, at a 16-byte aligned address and at an odd one: the result is that of the
    input alone, and the frame that ends at m under s = 1 and s = 2 reads its late rail's last value as 0, not the canary.  The
    outputs inside guard words, the CADUs at an aligned and at an odd address: the guards stay as they were."""
    import torch
    from meteor_demod_amd import frames
    st = L.LinkStream(seed=7, n_frames=4, lead=500, tail=0, differential=True)
    lib, stream = frames.lib(), C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    link = frames.make_link(True, True)
    for H in (12, 17):
        soft = st.received(H, 7.0, seed=70 + H)
        m = len(soft)
        rng = np.random.default_rng(shift)
        buf = np.where(rng.integers(0, 2, 4096 + 2 * m + 4096) > 0, 127, -127).astype(np.int8)
        start = 2048 + shift
        buf[start: start + 2 * m] = soft.reshape(-1)
        d = _dev(buf, gpu_device)
        src = C.c_void_p(d.data_ptr() + start)
        n_w = frames.windows(m, skew=True)
        guard = 0x5A5A5A5A
        cand = torch.full((4 * (n_w + 2),), guard, dtype=torch.int32, device=d.device)
        assert lib.mdemod_frames_link_candidates_device(C.byref(link), src, m, C.c_void_p(cand.data_ptr() + 16), gpu_device, stream) == 0
        c = cand.cpu().numpy().astype(np.int64)
        assert (c[:4] == guard).all() and (c[-4:] == guard).all()
        got = [frames.Candidate(int((r[0] & 0xFFFFFFFF) | (r[1] << 32)), int(r[3]), int(r[2])) for r in c[4:-4].reshape(-1, 4)]
        assert got == frames.model_candidates(soft, differential=True, skew=True)
        sent = [frames.Frame(p, H, 0, 0, 0, 0) for p in st.positions]
        assert sent[-1].position + FRAME == m
        arr = frames._to_c(sent)
        pad = 64 + (shift & 1) * 3                                            # the CADUs at an aligned address, or at an odd one
        out = torch.full((pad + len(sent) * 1024 + 64,), 0xA5, dtype=torch.uint8, device=d.device)
        assert lib.mdemod_frames_link_viterbi_device(C.byref(link), src, m, arr, len(sent), C.c_void_p(out.data_ptr() + pad), gpu_device, stream) == 0
        o = out.cpu().numpy()
        assert (o[:pad] == 0xA5).all() and (o[-64:] == 0xA5).all()
        mc, mf = frames.model_viterbi(soft, sent, differential=True, skew=True)
        print(f"shift {shift}, H {H}: channel_errors {[f.channel_errors for f in mf]}")
        assert np.array_equal(o[pad:-64].reshape(-1, 1024), mc) and frames._frames(arr, len(sent)) == mf
        assert [bytes(x) for x in mc] == st.frames


# ------------------------------------------------------------------------------------------------ the decoder on its own
def _hyps(sw):
    """The combined hypotheses a mode allows."""
    return [H for H in range(24 if sw["skew"] else 8) if not (sw["differential"] and H & 2)]


@pytest.mark.parametrize("differential,H", [(False, 9), (False, 18), (False, 21), (True, 5), (True, 9), (True, 16), (True, 15)])
def test_viterbi_is_maximum_likelihood(differential, H, gpu_device):
    """Two frames that tile a stream of 16 384 symbols at 2 dB (test_frames_link_host.py's streams; both skews, h swapped and not,
    H = 15 sent upside down and decoded as 13), decoded by the link kernel where they were sent: the bits of viterbi_ref's full-stream
    ML decoding (NRZ-M undone under `differential`), the decoder's own bits - the output coded again from the 0 before step 0 -
    with a path metric of M*, and the model's channel_errors (the header's count on the reference's d)."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    sw = dict(differential=differential, skew=True)
    st, soft, sym, d, best = V.ml_case(differential, H, 2.0)
    want = V.nrzm_undo(d) if differential else d
    sent = [frames.Frame(p, L.canonical(H, differential), 0, 0, 0, 0) for p in st.positions]
    cadu, fr = frames.viterbi(_dev(soft.copy(), gpu_device), sent, **sw)
    bits = V.bits_of(cadu.cpu().numpy())
    own = L.nrzm(bits) if differential else bits
    errors, differing, metric = int((want != st.bits).sum()), int((bits != want).sum()), V.path_metric(own, sym)
    print(f"H {H} ({_name(sw)}): {errors} of {len(d)} bits of the ML decoding differ from what was sent; kernel != ML in {differing}; M* {best}, the "
          f"kernel's path {metric}; channel_errors {[f.channel_errors for f in fr]}")
    assert errors >= 10
    assert metric == best
    assert differing == 0
    assert fr == frames.model_viterbi(soft, sent, **sw)[1]
    assert [f.channel_errors for f in fr] == [V.channel_errors(d[p: p + FRAME], sym[p: p + FRAME]) for p in st.positions]


@pytest.mark.parametrize("sw", SWITCHES, ids=_name)
@pytest.mark.parametrize("kind", ["zeros", "ties", "full", "signal"])
def test_viterbi_on_ties_and_full_scale(kind, sw, gpu_device):
    """8392 symbols the tracker would never call frames: all zeros (every bit is 0), symbols of -1 / 0 / 1, the full int8 range with
    -128; eight frames through eight of the mode's hypotheses in one launch, frames at 0 and at m - 8192 among them.  And a clean
    frame at +127 / -128 through hypotheses that negate a rail (-128 is negated in int32): the sent bytes and 0 channel errors.
    Bytes and channel_errors are the model's (which test_frames_link_host.py holds to the header's rule on these inputs)."""
    import viterbi_ref as V
    from meteor_demod_amd import frames
    hyps = _hyps(sw)
    if kind == "signal":
        st = L.LinkStream(seed=5, n_frames=1, lead=100, tail=100, differential=sw["differential"])
        cases = [(V.full_scale(st, H), [(100, H)]) for H in [H for H in hyps if H & 7 in (1, 4)][-3:]]
    else:
        cases = [(s, a) for name, s, a in V.hostile_inputs(tuple(hyps[::-3])) if name == kind]
    for soft, at in cases:
        assert len(soft) == V.HOSTILE_M
        sent = [frames.Frame(p, H, 0, 0, 0, 0) for p, H in at]
        cadu, fr = frames.viterbi(_dev(soft, gpu_device), sent, **sw)
        mc, mf = frames.model_viterbi(soft, sent, **sw)
        got = cadu.cpu().numpy()
        print(f"{kind} ({_name(sw)}): {int((soft == -128).sum())} values of -128; frames (position, H) {at}: ones per frame "
              f"{[int(V.bits_of(c).sum()) for c in got]}, channel_errors {[f.channel_errors for f in fr]}")
        assert np.array_equal(got, mc) and fr == mf
        if kind == "zeros":
            assert not got.any() and all(f.channel_errors == 0 for f in fr)
        if kind == "signal":
            assert (soft == -128).any() and bytes(got[0]) == st.frames[0] and fr[0].channel_errors == 0


def _viterbi_between_canaries(link, src, device, m, sent, odd, gpu_device):
    """mdemod_frames_link_viterbi_device on the m symbols at address `src` into a buffer of 0xA5 - the CADUs at an aligned address, or
    at an odd one - whose first and last bytes must stay as they were: (uint8 [n, 1024], the frames with channel_errors)."""
    import torch
    from meteor_demod_amd import frames
    arr = frames._to_c(sent)
    pad = 64 + 3 * odd
    out = torch.full((pad + len(sent) * 1024 + 64,), 0xA5, dtype=torch.uint8, device=device)
    st = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    rc = frames.lib().mdemod_frames_link_viterbi_device(C.byref(link), C.c_void_p(src), m, arr, len(sent), C.c_void_p(out.data_ptr() + pad), gpu_device, st)
    assert rc == 0
    o = out.cpu().numpy()
    assert (o[:pad] == 0xA5).all() and (o[-64:] == 0xA5).all()
    return o[pad:-64].reshape(-1, 1024), frames._frames(arr, len(sent))


@pytest.mark.parametrize("sw", SWITCHES, ids=_name)
def test_viterbi_takes_any_frame_list(sw, gpu_device):
    """Frame lists no tracker would make, on 2 x 8192 + 300 symbols: positions 0, 1, 127, 128, 129, 8191, m - 8192, a position twice,
    two frames that share one symbol, the mode's hypotheses in turn; the whole list, the list backwards, its first 1, 2 and 3 frames,
    and every frame alone; the CADUs at an aligned and at an odd address between canaries.  Bytes and channel_errors are the model's,
    the canaries stay, and a frame's result does not depend on what else is in the list."""
    from meteor_demod_amd import frames
    st = L.LinkStream(seed=9, n_frames=2, lead=150, tail=150, differential=sw["differential"])
    hyps = _hyps(sw)
    soft = st.received(hyps[-1], 3.0, seed=90)
    m = len(soft)
    assert m == 2 * FRAME + 300
    at = [0, 1, 127, 128, 129, FRAME - 1, m - FRAME, 128, 150, 150 + FRAME - 1, 0]
    sent = [frames.Frame(p, hyps[(k + 3) % len(hyps)] if k != 8 else hyps[-1], 0, 0, 0, 0) for k, p in enumerate(at)]
    mc, mf = frames.model_viterbi(soft, sent, **sw)
    d, link = _dev(soft, gpu_device), frames.make_link(**sw)
    run = lambda frames_, odd: _viterbi_between_canaries(link, d.data_ptr(), d.device, m, frames_, odd, gpu_device)   # noqa: E731
    for odd in (0, 1):
        cadu, fr = run(sent, odd)
        assert np.array_equal(cadu, mc) and fr == mf, odd
    cadu, fr = run(sent[::-1], 0)
    assert np.array_equal(cadu, mc[::-1]) and fr == mf[::-1]
    for n in (1, 2, 3):
        cadu, fr = run(sent[:n], n & 1)
        assert np.array_equal(cadu, mc[:n]) and fr == mf[:n], n
    for k, f in enumerate(sent):
        cadu, fr = run([f], k & 1)
        assert np.array_equal(cadu[0], mc[k]) and fr == [mf[k]], k
    print(f"{_name(sw)}, m {m}: {len(sent)} frames (position, H) {[(f.position, f.hypothesis) for f in sent]}, channel_errors {[f.channel_errors for f in mf]}; "
          f"the frame at 150, which is where and as one was sent, comes back as sent: {bytes(mc[8]) == st.frames[0]}")


@pytest.mark.parametrize("differential", [False, True])
@pytest.mark.parametrize("H", [8, 9, 16, 17])
def test_viterbi_at_the_ends_of_the_stream(H, differential, gpu_device):
    """Two frames and nothing else at 3 dB, the stream at an odd address between canaries of +-127.  The frame at m - 8192 under s = 1
    and s = 2 with h even and odd reads its late rail at index m, which is 0 and not the canary: the symbol that follows the stream
    reads +127 on both rails through h, so that channel_errors would count it (a hard decision of 0 is "not positive").  The frame
    at 0 has no lead-in, and with `differential` no bit before step 0.  Bytes and channel_errors are the model's, for both frames
    in one launch and for each alone."""
    from meteor_demod_amd import frames
    sw = dict(differential=differential, skew=True)
    st = L.LinkStream(seed=7, n_frames=2, lead=0, tail=0, differential=differential)
    soft = st.received(H, 3.0, seed=70 + H)
    m = len(soft)
    buf = np.where(np.random.default_rng(H).integers(0, 2, 4096 + 2 * m + 4096) > 0, 127, -127).astype(np.int8)
    start = 2048 + 1001
    buf[start: start + 2 * m] = soft.reshape(-1)
    buf[start + 2 * m: start + 2 * m + 2] = U.through_inverse(np.array([[127, 127]]), H & 7)[0]
    d, link = _dev(buf, gpu_device), frames.make_link(**sw)
    sent = [frames.Frame(0, H, 0, 0, 0, 0), frames.Frame(m - FRAME, H, 0, 0, 0, 0)]
    mc, mf = frames.model_viterbi(soft, sent, **sw)
    cadu, fr = _viterbi_between_canaries(link, d.data_ptr() + start, d.device, m, sent, 1, gpu_device)
    wrong = [int((np.unpackbits(c) != np.unpackbits(np.frombuffer(f, dtype=np.uint8))).sum()) for c, f in zip(cadu, st.frames)]
    print(f"H {H} ({_name(sw)}): channel_errors {[f.channel_errors for f in fr]}, bits that differ from what was sent {wrong}")
    assert np.array_equal(cadu, mc) and fr == mf
    for k in (0, 1):
        alone, fa = _viterbi_between_canaries(link, d.data_ptr() + start, d.device, m, [sent[k]], 0, gpu_device)
        assert np.array_equal(alone[0], mc[k]) and fa == [mf[k]]


# ---------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("piece", [8192, 16384])
def test_host_entry_in_pieces_equals_the_device_entry(piece, gpu_device):
    """The skew-change stream (two runs, 66 000 symbols) and a stream whose frames end at m through mdemod_frames_link_decode_host
    in pieces of 16 384 (and 8 192) symbols: the frame list and the bytes of mdemod_frames_link_decode_device on the whole stream."""
    from meteor_demod_amd import frames
    sw = dict(differential=True, skew=True)
    for k in (2, 0, 1):
        _, soft, n = list(_edge_streams())[k]
        whole = frames.decode(_dev(soft, gpu_device), **sw)
        parts = frames.decode(soft, piece_symbols=piece, device=gpu_device, **sw)
        assert len(whole[1]) == n
        _same(parts, whole)
        _same(frames.decode(soft, device=gpu_device, **sw), whole)            # (one piece)
    st = L.LinkStream(seed=1)
    soft = st.received(21, 3.0, seed=9)
    _same(frames.decode(soft, piece_symbols=piece, device=gpu_device, skew=True), frames.decode(_dev(soft, gpu_device), skew=True))


# ---------------------------------------------------------------------------------------------------------- switches off
def test_switches_off_is_the_plain_layer(gpu_device):
    """The link entries with a zeroed mdemod_frames_link (and with NULL) against the plain entries on the plain tests' stream."""
    import torch
    from meteor_demod_amd import frames
    soft = U.Stream(seed=1).received(3, 3.0, seed=203)
    m = len(soft)
    d = _dev(soft, gpu_device)
    lib, stream = frames.lib(), C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    off = frames.MdemodFramesLink()
    cap = m // FRAME
    plain_c = frames.candidates_tensor(d)
    plain = frames.decode(d)
    sent = [frames.Frame(777 + FRAME * k, 3, 0, 0, 0, 0) for k in range(5)]
    plain_v = frames.viterbi(d, sent)
    for link in (C.byref(off), None):
        assert lib.mdemod_frames_link_windows(link, m) == frames.windows(m)
        c = torch.zeros_like(plain_c)
        assert lib.mdemod_frames_link_candidates_device(link, C.c_void_p(d.data_ptr()), m, C.c_void_p(c.data_ptr()), gpu_device, stream) == 0
        assert torch.equal(c, plain_c)
        arr = frames._to_c(sent)
        out = torch.zeros((5, 1024), dtype=torch.uint8, device=d.device)
        assert lib.mdemod_frames_link_viterbi_device(link, C.c_void_p(d.data_ptr()), m, arr, 5, C.c_void_p(out.data_ptr()), gpu_device, stream) == 0
        assert torch.equal(out, plain_v[0]) and frames._frames(arr, 5) == plain_v[1]
        for host in (False, True):
            info, cadu, n = (frames.MdemodFrameInfo * cap)(), np.zeros((cap, 1024), dtype=np.uint8), C.c_uint64()
            if host:
                rc = lib.mdemod_frames_link_decode_host(link, None, soft.ctypes.data, m, cadu.ctypes.data, info, cap, C.byref(n), gpu_device)
            else:
                rc = lib.mdemod_frames_link_decode_device(link, None, C.c_void_p(d.data_ptr()), m, cadu.ctypes.data, info, cap, C.byref(n), gpu_device, stream)
            assert rc == 0
            _same((cadu[: n.value], frames._frames(info, n.value)), plain)
        arr = frames._to_c([frames.Frame(777, 8, 0, 0, 0, 0)])
        assert lib.mdemod_frames_link_viterbi_device(link, C.c_void_p(d.data_ptr()), m, arr, 1, C.c_void_p(out.data_ptr()), gpu_device, stream) != 0


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def runs(gpu_device):
    """The recording at its four starting phases through the GPU OQPSK demodulator and the GPU link layer, once: phase -> (soft,
    CADUs, frames)."""
    from meteor_demod_amd import Demodulator, frames
    out = {}
    for phase in L.REC_PHASES:
        _, iq = L.recording(phase)
        with Demodulator(L.recording_cfg(), 1, gpu_device) as dm:
            soft = dm.process_host([iq])[0]
        out[phase] = (soft, *frames.decode(_dev(soft, gpu_device), skew=True, differential=True))
    return out


@pytest.mark.parametrize("phase", L.REC_PHASES)
def test_oqpsk_recording_through_the_gpu_demodulator_and_the_link_layer(phase, runs):
    """9 NRZ-M frames as OQPSK (RRC 0.6, 4 samples per symbol, 0 Hz, about 13 dB) at a starting carrier phase of `phase` turns
    through the GPU OQPSK demodulator, then decode(skew=True, differential=True): no frame is left out but those that begin before
    the CPU run's lock symbol, every recovered frame is what was sent, and the GPU result equals the CPU result (reference
    demodulator + host model) frame for frame.  (On the CPU the reference's demodulation of this recording locks at symbol 3235 /
    3181 and yields all nine frames at every phase: the seeds do not sit on one of its false locks.)"""
    st, _ = L.recording(phase)
    cpu_soft, lock, cpu_cadu, cpu_fr = L.recording_cpu(phase)
    assert lock is not None
    soft, cadu, fr = runs[phase]
    print(f"phase {phase}: {len(soft)} symbols (CPU: {len(cpu_soft)}), lock at {lock}, {len(fr)} frames (CPU: {len(cpu_fr)}), (h, s) "
          f"{sorted({(f.hypothesis & 7, f.hypothesis >> 3) for f in fr})}, channel_errors {[f.channel_errors for f in fr]}; soft symbols equal to the "
          f"CPU's: {len(soft) == len(cpu_soft) and np.array_equal(soft, cpu_soft)}")
    got = [bytes(c) for c in cadu]
    assert got == [bytes(c) for c in cpu_cadu] and [(f.position, f.hypothesis) for f in fr] == [(f.position, f.hypothesis) for f in cpu_fr]
    assert all(g in st.frames for g in got)
    delay = fr[0].position - st.positions[st.frames.index(got[0])]
    assert 0 <= delay < 64
    due = [k for k, p in enumerate(st.positions) if p + delay >= lock and p + delay + FRAME + 1 <= len(soft)]
    assert len(due) >= 6 and all(st.frames[k] in got for k in due), (due, [st.frames.index(g) for g in got])


def test_oqpsk_recording_meets_unskewed_and_skewed_locks(runs):
    """Over the four phases above, both a lock without skew and one with skew occur (profiles/frames_link.md records which)."""
    pairs = {phase: sorted({(f.hypothesis & 7, f.hypothesis >> 3) for f in fr}) for phase, (_, _, fr) in runs.items()}
    print(f"(h, s) per phase: {pairs}")
    skews = {s for v in pairs.values() for _, s in v}
    assert 0 in skews and skews - {0}


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_oqpsk_skew_diff(tmp_path, gpu_device):
    """-m oqpsk --cadu --vcdu --skew --diff on the recording, its frames Reed-Solomon coded and randomised, as a WAV: the .cadu holds
    the bytes of frames.decode_file(skew, differential) on the .s, and the transfer-frame layer finds 0 uncorrectable."""
    from conftest import ROOT
    from meteor_demod_amd import frames
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    st, iq = L.recording(0.0, True)
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    out = tmp_path / "pass.s"
    p = subprocess.run([str(cli_exe), "-q", "-B", "-m", "oqpsk", "--device", str(gpu_device), "--cadu", "--vcdu", "--skew", "--diff", "-o", str(out), str(wav)],
                       capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    data, rep = frames.decode_file(out, device=gpu_device, skew=True, differential=True)
    got = (tmp_path / "pass.cadu").read_bytes()
    assert rep.frames >= 6 and len(got) == 1024 * rep.frames and got == data
    assert all(got[k: k + 1024] in st.frames for k in range(0, len(got), 1024))
    lines = p.stdout.strip().splitlines()
    assert f"{rep.frames} frames ({rep.flywheel_frames} flywheel) in {rep.runs} runs" in lines[-2]
    assert f"{rep.frames} frames, 0 uncorrectable" in lines[-1]
    assert len((tmp_path / "pass.vcdu").read_bytes()) == 892 * rep.frames
    plain = subprocess.run([str(cli_exe), "-q", "-B", "-m", "oqpsk", "--device", str(gpu_device), "--cadu", "-o", str(tmp_path / "plain.s"), str(wav)],
                           capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert plain.returncode == 0 and (tmp_path / "plain.s").read_bytes() == out.read_bytes()
    assert (tmp_path / "plain.cadu").read_bytes() != got                     # (without the flags nothing changed: the plain layer, which finds none of it)
