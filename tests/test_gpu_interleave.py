"""GPU tests of the 80 k interleaved mode (include/meteor_demod_amd_interleave.h): the two kernels of csrc/interleave.hip against the
host model, byte for byte - the sync search at the edges of a stream, on random symbols, under all 24 hypotheses, with the input at
an odd symbol offset inside garbage and the output inside canaries; the gather for three branch delays over the slip stream, with
the tracker's segments, hand-made tables (one segment; more than travel as kernel arguments) and the output inside canaries; the
device entry against the host entry; Reed-Solomon coded frames end to end at the default branch delay; and the keywords on
frames.decode and rs.soft_to_vcdu.  Every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import interleave_util as IU

pytestmark = pytest.mark.gpu

W = IU.WINDOW
EDGES = [0, 3, 4, 5, 2562, 2563, 2564, 5123, 3 * W + 17]


def _dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{gpu_device}")


def _stream(gpu_device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)


# ------------------------------------------------------------------------------------------------------------ sync search
@pytest.mark.parametrize("kind", ["full", "ties"])
@pytest.mark.parametrize("m", EDGES)
def test_candidates_equal_the_model(m, kind, gpu_device):
    """Random int8 over the full range, -128 included (and symbols of -1 / 0 / 1, where most sums tie), at the lengths where the
    window count and the last window's positions change: one candidate per window, equal to the model's in position, hypothesis
    and score."""
    from meteor_demod_amd import interleave as il
    rng = np.random.default_rng(m + len(kind))
    soft = rng.integers(-128, 128, (m, 2)).astype(np.int8) if kind == "full" else rng.integers(-1, 2, (m, 2)).astype(np.int8)
    if kind == "full" and m:
        soft[rng.integers(0, m, m // 16 + 1)] = -128
    want = il.model_candidates(soft)
    got = il.candidates(_dev(soft, gpu_device))
    print(f"m {m} ({kind}): {len(got)} windows, {got[:4]}")
    assert len(got) == il.windows(m) == len(want) and got == want


@pytest.mark.parametrize("shift", [0, 2, 14])
def test_candidates_under_all_hypotheses_inside_garbage(shift, gpu_device):
    """An interleaved stream at 3 dB through each of the 24 H (three full windows and a short one), the input at an even and at an odd
    symbol offset inside garbage of +-127, the output inside canaries: the model's candidates, (phase, H) of the sender in every
    full window, and the canaries as they were."""
    import torch
    from meteor_demod_amd import interleave as il
    snd = IU.random_sender(200, 3 * 64 + 9, 2, lead=21)
    guard = 0x5A5A5A5A
    for H in range(24):
        soft = snd.received(H, 3.0, seed=2000 + H)
        m = len(soft)
        rng = np.random.default_rng(H)
        buf = np.where(rng.integers(0, 2, 4096 + 2 * m + 4096) > 0, 127, -127).astype(np.int8)
        start = 2048 + shift
        buf[start: start + 2 * m] = soft.reshape(-1)
        d = _dev(buf, gpu_device)
        n_w = il.windows(m)
        cand = torch.full((4 * (n_w + 2),), guard, dtype=torch.int32, device=d.device)
        assert il.lib().mdemod_il_candidates_device(C.c_void_p(d.data_ptr() + start), m, C.c_void_p(cand.data_ptr() + 16), gpu_device, _stream(gpu_device)) == 0
        c = cand.cpu().numpy().astype(np.int64)
        assert (c[:4] == guard).all() and (c[-4:] == guard).all()
        got = il._cands_of(c[4:-4])
        assert got == il.model_candidates(soft), H
        assert [(g.position - W * w, g.hypothesis) for w, g in enumerate(got[:3])] == [(21, H)] * 3, (H, got)
    print(f"shift {shift}: 24 H, {n_w} windows each, the last candidate {got[-1]}")


def test_candidates_refuse_an_odd_address(gpu_device):
    from meteor_demod_amd import _capi, interleave as il
    import torch
    d = torch.zeros(4096, dtype=torch.int8, device=f"cuda:{gpu_device}")
    cand = torch.zeros(16, dtype=torch.int32, device=d.device)
    rc = il.lib().mdemod_il_candidates_device(C.c_void_p(d.data_ptr() + 1), 1000, C.c_void_p(cand.data_ptr()), gpu_device, _stream(gpu_device))
    assert rc == _capi.MDEMOD_ERR_PARAM and "odd address" in _capi.last_error()


# ------------------------------------------------------------------------------------------------------------- the gather
@pytest.fixture(scope="module")
def slip():
    """The slip stream (3000 periods and 18 symbols: not a multiple of 40) with the model's candidates and the tracker's segments."""
    from meteor_demod_amd import interleave as il
    snd = IU.slip_sender(8)
    soft = snd.received(IU.SLIP_H[0], None, seed=3)
    segs, P = il.track(il.model_candidates(soft), len(soft))
    assert len(soft) % 40 and len(segs) == 4 and P == 3000
    return snd, soft, segs, P


def _tables(il, segs, P, m):
    yield "the tracker's four segments", segs, P
    yield "one hand-made segment", [il.Segment(0, 23, 0, 23, 13)], (m - 23) // 40
    many = [il.Segment(0, 5 + 2801 * i, 70 * i, 5, (7 * i) % 24) for i in range(40)]
    yield "forty hand-made segments (a table in device memory)", many, 2950
    yield "thirty-two segments (the most that travel as kernel arguments)", many[:32], 2400
    yield "thirty-three segments", many[:33], 2400


@pytest.mark.parametrize("M", [1, 8, 2048])
def test_gather_equals_the_model(M, slip, gpu_device):
    """The gather over the slip stream for three branch delays and five segment tables, the output inside canaries at an aligned
    and at an odd address: the model's bytes, the canaries as they were.  At M = 8 and the tracker's segments the bits are the
    sender's."""
    import torch
    from meteor_demod_amd import interleave as il
    snd, soft, segs, P = slip
    m = len(soft)
    d = _dev(soft, gpu_device)
    o = il.make_opts(branch_delay=M)
    for k, (name, table, periods) in enumerate(_tables(il, segs, P, m)):
        want = il.model_deinterleave(soft, table, periods, branch_delay=M)
        pad = 64 + (k & 1) * 3
        out = torch.full((pad + 72 * periods + 64,), 0x5A, dtype=torch.int8, device=d.device)
        rc = il.lib().mdemod_il_deinterleave_device(C.byref(o), C.c_void_p(d.data_ptr()), m, il._segs_to_c(table), len(table), periods,
                                                    C.c_void_p(out.data_ptr() + pad), gpu_device, _stream(gpu_device))
        assert rc == 0
        got = out.cpu().numpy()
        assert (got[:pad] == 0x5A).all() and (got[-64:] == 0x5A).all()
        zeros = int((want == 0).sum())
        print(f"M {M}, {name}: {72 * periods} bytes, {zeros} of them 0")
        assert np.array_equal(got[pad:-64], want.reshape(-1)), name
        assert np.array_equal(il.deinterleave(d, table, periods, branch_delay=M).cpu().numpy(), want)
    if M == 8:
        compared, excluded, n = IU.check_bits(snd, il.deinterleave(d, segs, P, branch_delay=8).cpu().numpy(), P)
        print(f"M 8: {compared} bits right, {excluded} of {n} near an event")
        assert excluded / n <= 0.30


def test_gather_refusals(slip, gpu_device):
    import torch
    from meteor_demod_amd import _capi, interleave as il
    _, soft, segs, P = slip
    d = _dev(soft, gpu_device)
    with pytest.raises(_capi.MdemodError):
        il.deinterleave(d, [il.Segment(0, 3, 1, 3, 5)], 100)
    with pytest.raises(_capi.MdemodError):
        il.deinterleave(d, segs[:1] + [il.Segment(0, 3, 5, 3, 24)], 100)
    o = il.make_opts()
    rc = il.lib().mdemod_il_deinterleave_device(C.byref(o), C.c_void_p(d.data_ptr()), len(soft), il._segs_to_c(segs), len(segs), 100,
                                                C.c_void_p(d.data_ptr() + 1000), gpu_device, _stream(gpu_device))
    assert rc == _capi.MDEMOD_ERR_PARAM and "overlap" in _capi.last_error()
    assert tuple(il.deinterleave(d, [], 0).shape) == (0, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ all three steps
def test_decode_device_equals_decode_host_and_the_model(slip, gpu_device):
    from meteor_demod_amd import interleave as il
    snd, soft, segs, P = slip
    want, wsegs, wP = il.model_decode(soft, branch_delay=8)
    dev_out, dev_rep = il.decode(_dev(soft, gpu_device), branch_delay=8)
    host_out, host_rep = il.decode(soft, branch_delay=8, device=gpu_device)
    print(f"{dev_rep.segments} segments, {dev_rep.periods} periods, mean sync score {dev_rep.mean_score} of {il.FULL_SCORE}")
    assert dev_rep == host_rep and dev_rep.list == wsegs == segs and dev_rep.periods == wP == P and dev_rep.symbols == len(soft)
    assert np.array_equal(dev_out.cpu().numpy(), want) and np.array_equal(host_out, want)
    assert 0.9 * il.FULL_SCORE < dev_rep.mean_score <= il.FULL_SCORE
    # a short output buffer takes the first symbols of the same gather; noise gives no segment and nothing to write
    import torch
    room = 36 * 1000 + 35
    out = torch.full((2 * room + 64,), 0x5A, dtype=torch.int8, device=f"cuda:{gpu_device}")
    seg_arr, n, p, mean = (il.MdemodIlSegment * 2)(), C.c_uint64(), C.c_uint64(), C.c_int32()
    o = il.make_opts(branch_delay=8)
    d = _dev(soft, gpu_device)
    assert il.lib().mdemod_il_decode_device(C.byref(o), C.c_void_p(d.data_ptr()), len(soft), C.c_void_p(out.data_ptr()), room, seg_arr, 2, C.byref(n),
                                            C.byref(p), C.byref(mean), gpu_device, _stream(gpu_device)) == 0
    got = out.cpu().numpy()
    assert (n.value, p.value) == (4, P) and il._segments(seg_arr, 2) == segs[:2]
    assert np.array_equal(got[: 72 * 1000], want.reshape(-1)[: 72 * 1000]) and (got[72 * 1000:] == 0x5A).all()
    import frames_util as U
    noise = U.noise(5 * W, seed=9)
    out, rep = il.decode(_dev(noise, gpu_device))
    assert tuple(out.shape) == (0, 2) and (rep.segments, rep.periods) == (0, 0)
    out, rep = il.decode(noise, device=gpu_device)
    assert out.shape == (0, 2) and (rep.segments, rep.periods) == (0, 0)


@pytest.fixture(scope="module")
def framed():
    """Four RS-coded frames interleaved with M = 8 at 6 dB through the inverse of H = 20, and what the models make of them."""
    from meteor_demod_amd import frames, interleave as il
    out = {}
    for differential in (False, True):
        snd = IU.FramedSender(seed=50, M=8, n_frames=4, tail_bits=IU.tail_bits_for(8, 4, 777), differential=differential, lead=11)
        soft = snd.received(20, 6.0, seed=80)
        out[differential] = (snd, soft, frames.model_decode(il.model_decode(soft, branch_delay=8)[0], differential=differential))
    return out


@pytest.mark.parametrize("differential", [False, True], ids=["plain", "differential"])
def test_frames_decode_with_interleaved(differential, framed, gpu_device):
    """frames.decode(interleaved=True, branch_delay=8) on a device tensor and on a numpy array: the CADUs and the frame list of the
    models, and the frames that were sent; skew=True beside it changes nothing."""
    from meteor_demod_amd import frames
    snd, soft, (want_cadu, want_fr) = framed[differential]
    for src in (_dev(soft, gpu_device), soft):
        kw = dict(device=gpu_device) if isinstance(src, np.ndarray) else {}
        cadu, fr = frames.decode(src, interleaved=True, branch_delay=8, differential=differential, **kw)
        assert fr == want_fr and np.array_equal(cadu, want_cadu)
        cadu2, fr2 = frames.decode(src, interleaved=True, branch_delay=8, differential=differential, skew=True, **kw)
        assert fr2 == fr and np.array_equal(cadu2, cadu)
    print(f"differential {differential}: frames at {[f.position for f in fr]}, channel_errors {[f.channel_errors for f in fr]}")
    assert [bytes(c) for c in cadu] == snd.frames and [f.position for f in fr] == snd.positions


def test_end_to_end_at_the_default_branch_delay(gpu_device):
    """Four RS-coded frames early in a stream of about 1.47 M symbols interleaved with M = 2048 (frames' end + 35 x 36 x 2048 bits
    <= stream length: all their sources exist), through the inverse of H = 9 at Es/N0 = 6 dB, through
    rs.soft_to_vcdu(interleaved=True): the VCDUs that were sent, 0 uncorrectable."""
    from meteor_demod_amd import rs
    snd = IU.FramedSender(seed=51, M=2048, n_frames=4, tail_bits=IU.tail_bits_for(2048, 4, 777), lead=7)
    assert 2 * (snd.positions[-1] + 8192) + 35 * 36 * 2048 <= len(snd.u)
    soft = snd.received(9, 6.0, seed=81)
    vcdu, info, fr = rs.soft_to_vcdu(_dev(soft, gpu_device), interleaved=True)
    rep = rs.report(vcdu.cpu().numpy(), info.cpu().numpy())
    print(f"{len(soft)} symbols, {len(fr)} frames at {[f.position for f in fr]} as h {sorted({f.hypothesis for f in fr})}, channel_errors "
          f"{[f.channel_errors for f in fr]}, {rep.bytes_corrected} bytes corrected, {rep.uncorrectable_frames} uncorrectable")
    assert [f.position for f in fr] == snd.positions and {f.hypothesis for f in fr} == {0}
    assert rep.uncorrectable_frames == 0 and [bytes(v) for v in vcdu.cpu().numpy()] == [bytes(v) for v in snd.vcdus]


def test_interleaved_false_is_the_call_without_the_keyword(gpu_device):
    import rs_util
    import torch
    from meteor_demod_amd import frames, rs
    soft = rs_util.stream().received(3, 6.0, seed=5)
    d = _dev(soft, gpu_device)
    a, b = frames.decode(d), frames.decode(d, interleaved=False, branch_delay=8)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and len(a[1]) == 5
    a, b = frames.decode(soft, device=gpu_device), frames.decode(soft, device=gpu_device, interleaved=False)
    assert a[1] == b[1] and np.array_equal(a[0], b[0])
    a, b = rs.soft_to_vcdu(d), rs.soft_to_vcdu(d, interleaved=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    with pytest.raises(TypeError):
        frames.decode(d, interleaved=1)
