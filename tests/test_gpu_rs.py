"""GPU tests of the transfer-frame layer (include/meteor_demod_amd_rs.h): the kernel against the host model, byte for byte, on
batches whose codewords carry every kind of load side by side; guard regions; the entries' argument checks; the pieces of the host
entry; noisy framed streams through the Viterbi decoder and this layer; and the C host's --vcdu.  Every test prints the figures it
asserts on."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import frames_util as U
import rs_util as R

pytestmark = pytest.mark.gpu


def _dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{gpu_device}")


def _stream_handle(gpu_device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)


# ------------------------------------------------------------------------------------------------------ kernel against model
@pytest.mark.parametrize("opts", R.OPTS, ids=str)
@pytest.mark.parametrize("n", [1, 2, 5, 67])
def test_kernel_equals_the_model(n, opts, gpu_device):
    """Per-codeword loads of 0, 1, 2, 8, 15, 16, 17 and 32 errors, parity-only errors and whole random frames, mixed so that the
    waves of a block and neighbouring blocks take different paths: VCDUs and reports are the model's, and every corrected codeword
    is the bytes that were encoded."""
    from meteor_demod_amd import rs
    sent, cadu, loads = R.mixed_batch(n, seed=100 + n, **opts)
    want_v, want_i = rs.model_decode(cadu, **opts)
    got_v, got_i = rs.decode(_dev(cadu, gpu_device), **opts)
    got_v, got_i = got_v.cpu().numpy(), got_i.cpu().numpy()
    print(f"n {n} {opts}: loads of frame 0 {loads[0]}, reports {got_i[: min(n, 4), :5].tolist()}; frames flagged {int(got_i[:, 4].sum())}")
    assert got_i.shape == (n, 8) and np.array_equal(got_i, want_i)
    assert got_v.shape == (n, 892) and np.array_equal(got_v, want_v)
    R.check_against_what_was_sent(sent, cadu, loads, got_v, got_i, **opts)


def test_every_single_error_position_on_the_gpu(gpu_device):
    """One error at each position 0 .. 254 (the ends of the Chien search, the data / parity border, every lane and every q)."""
    from meteor_demod_amd import rs
    rng = np.random.default_rng(21)
    v = R.vcdu(rng)
    clean = rs.model_encode(v)
    batch = np.stack([clean] * 255)
    for p in range(255):
        batch[p, 4 + 4 * p + p % 4] ^= np.uint8(1 + p % 255)
    got_v, got_i = rs.decode(_dev(batch, gpu_device))
    got_v, got_i = got_v.cpu().numpy(), got_i.cpu().numpy()
    want = np.zeros((255, 8), dtype=np.uint8)
    want[np.arange(255), np.arange(255) % 4] = 1
    assert (got_v == v).all() and np.array_equal(got_i, want)


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """The input inside garbage on both sides: the result is that of the input alone.  The outputs between canaries: they survive."""
    import torch
    from meteor_demod_amd import rs
    n = 5
    _, cadu, _ = R.mixed_batch(n, seed=31)
    rng = np.random.default_rng(shift)
    buf = rng.integers(0, 256, 4096 + n * 1024 + 4096, dtype=np.uint8)
    start = 2048 + shift
    buf[start: start + n * 1024] = cadu.reshape(-1)
    d = _dev(buf, gpu_device)
    pad = 64 + shift % 64
    out = torch.full((pad + n * 892 + 64,), 0xA5, dtype=torch.uint8, device=d.device)
    info = torch.full((16 + n * 8 + 16,), 0x5A, dtype=torch.uint8, device=d.device)
    rc = rs.lib().mdemod_rs_decode_device(None, C.c_void_p(d.data_ptr() + start), n, C.c_void_p(out.data_ptr() + pad), C.c_void_p(info.data_ptr() + 16),
                                          gpu_device, _stream_handle(gpu_device))
    assert rc == 0
    o, i = out.cpu().numpy(), info.cpu().numpy()
    assert (o[:pad] == 0xA5).all() and (o[-64:] == 0xA5).all() and (i[:16] == 0x5A).all() and (i[-16:] == 0x5A).all()
    want_v, want_i = rs.model_decode(cadu)
    assert np.array_equal(o[pad:-64].reshape(n, 892), want_v) and np.array_equal(i[16:-16].reshape(n, 8), want_i)
    assert np.array_equal(d.cpu().numpy(), buf)                               # the input is only read


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    import torch
    from meteor_demod_amd import _capi, rs
    lib, st = rs.lib(), _stream_handle(gpu_device)
    assert lib.mdemod_rs_decode_device(None, None, 0, None, None, gpu_device, st) == 0                      # n = 0: nothing to do
    v, i = rs.decode(torch.zeros((0, 1024), dtype=torch.uint8, device=f"cuda:{gpu_device}"))
    assert tuple(v.shape) == (0, 892) and tuple(i.shape) == (0, 8)
    assert rs.decode(np.zeros((0, 1024), dtype=np.uint8), device=gpu_device)[0].shape == (0, 892)
    n = 3
    buf = torch.zeros(n * 1024 + n * 892 + n * 8 + 64, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    cadu, vcdu, info = base, base + n * 1024, base + n * 1024 + n * 892

    def refused(word, opts, a, b, c):
        rc = lib.mdemod_rs_decode_device(C.byref(opts) if opts is not None else None, C.c_void_p(a), n, C.c_void_p(b), C.c_void_p(c), gpu_device, st)
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text

    assert lib.mdemod_rs_decode_device(None, C.c_void_p(cadu), n, C.c_void_p(vcdu), C.c_void_p(info), gpu_device, st) == 0
    refused("intersect", None, cadu, cadu + 1024 * n - 4, info)               # the VCDUs begin in the last CADU
    refused("intersect", None, cadu, cadu, info)                              # in place
    refused("intersect", None, cadu, vcdu, cadu + 512)                        # the report inside the input
    refused("intersect", None, cadu, vcdu, vcdu + 892 * n - 8)                # the report inside the VCDUs
    refused("needed", None, 0, vcdu, info)
    refused("needed", None, cadu, 0, info)
    refused("needed", None, cadu, vcdu, 0)
    refused("multiples of 4", None, cadu, vcdu + 2, info)
    refused("derandomise", rs.make_opts(derandomise=2), cadu, vcdu, info)
    refused("dual_basis", rs.make_opts(dual_basis=3), cadu, vcdu, info)
    refused("piece_frames", rs.make_opts(piece_frames=(1 << 20) + 1), cadu, vcdu, info)
    with pytest.raises(_capi.MdemodError) as e:
        rs.decode(np.zeros((2, 1024), dtype=np.uint8), dual_basis=2, device=gpu_device)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "dual_basis" in e.value.detail
    torch.cuda.synchronize(gpu_device)


# ---------------------------------------------------------------------------------------------------------------- pieces
def test_host_entry_in_pieces_equals_the_device_entry(gpu_device):
    """5 frames through mdemod_rs_decode_host in pieces of 2 (2 + 2 + 1): the bytes of mdemod_rs_decode_device on all 5."""
    from meteor_demod_amd import rs
    _, cadu, _ = R.mixed_batch(5, seed=41)
    whole_v, whole_i = rs.decode(_dev(cadu, gpu_device))
    whole_v, whole_i = whole_v.cpu().numpy(), whole_i.cpu().numpy()
    for piece in (2, 0, 5, 1):
        v, i = rs.decode(cadu, piece_frames=piece, device=gpu_device)
        assert np.array_equal(v, whole_v) and np.array_equal(i, whole_i), piece
    assert whole_i[:, 4].any() and not whole_i[:, 4].all()


# --------------------------------------------------------------------------------------------------------------- streams
def test_stream_at_2_db_every_frame_is_repaired(gpu_device):
    """Five RS-encoded frames at Es/N0 = 2 dB, Viterbi-decoded at the sent positions, all eight hypotheses (receive seeds 200 + h):
    the inner decoder leaves byte errors in every frame (expected: at most about 8 in a codeword, the code takes 16); every VCDU
    comes out as sent, no frame is flagged."""
    from meteor_demod_amd import frames, rs
    st = R.stream()
    worst = 0
    for h in range(8):
        soft = _dev(st.received(h, 2.0, seed=200 + h), gpu_device)
        cadu, _ = frames.viterbi(soft, [frames.Frame(p, h, 0, 0, 0, 0) for p in st.positions])
        damaged = sum(bytes(c) != f for c, f in zip(cadu.cpu().numpy(), st.frames))
        vcdu, info = rs.decode(cadu)
        vcdu, info = vcdu.cpu().numpy(), info.cpu().numpy()
        per_frame = info[:, :4].astype(int).sum(axis=1)
        print(f"h {h}: {damaged} of 5 CADUs with byte errors; corrected per frame {per_frame.tolist()}, worst codeword {int(info[:, :4].max())}")
        assert [bytes(v) for v in vcdu] == [bytes(v) for v in st.vcdus], h
        assert not info[:, 4:].any() and (per_frame > 0).all(), h
        worst = max(worst, int(info[:, :4].max()))
    print(f"worst codeword over the eight hypotheses: {worst} byte errors (limit 16)")
    assert worst <= 16


def test_stream_at_3_db_through_soft_to_vcdu(gpu_device):
    """The same frames at 3 dB through sync search, tracker, Viterbi and this layer without leaving the device: every tracked frame is
    one that was sent, at its position, and exact."""
    from meteor_demod_amd import rs
    st = R.stream()
    for h in range(8):
        vcdu, info, found = rs.soft_to_vcdu(_dev(st.received(h, 3.0, seed=300 + h), gpu_device))
        assert vcdu.is_cuda and info.is_cuda and tuple(vcdu.shape) == (len(found), 892)
        vcdu, info = vcdu.cpu().numpy(), info.cpu().numpy()
        print(f"h {h}: {len(found)} frames tracked, corrected {info[:, :4].astype(int).sum(axis=1).tolist()}")
        assert len(found) >= 1 and all(f.position in st.positions and f.hypothesis == h for f in found)
        for k, f in enumerate(found):
            assert bytes(vcdu[k]) == bytes(st.vcdus[st.positions.index(f.position)]), (h, k)
        assert not info[:, 4:].any()


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_vcdu(tmp_path, gpu_device):
    """--cadu --vcdu on the 9-frame recording, re-made with encoded frames: the .vcdu is rs.model_decode of the .cadu, its frames (all
    after the lock, at least 6 consecutive ones of the 9) are the VCDUs that were sent, and the summary line says what the report says.
    --vcdu alone writes the same .vcdu and no .cadu."""
    from conftest import ROOT
    from meteor_demod_amd import rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    st, iq = R.recording()
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    out = tmp_path / "pass.s"
    p = subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), "--cadu", "--vcdu", "-o", str(out), str(wav)], capture_output=True,
                       text=True, cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    cadu = np.frombuffer((tmp_path / "pass.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    got = (tmp_path / "pass.vcdu").read_bytes()
    want_v, want_i = rs.model_decode(cadu)
    assert len(cadu) >= 6 and got == want_v.tobytes()
    # the .s of the C host begins shortly before the lock (the reference's ring of 512 symbols), so every frame of the files lies
    # after it; which of the nine each one is, its own counter says: consecutive ones, and each frame the VCDU sent under that counter
    counters = [rs.header(got[892 * k: 892 * k + 5]).counter for k in range(len(cadu))]
    print(f"{len(cadu)} frames, counters {counters}")
    assert counters == list(range(counters[0], counters[0] + len(cadu))) and counters[-1] < U.REC_FRAMES
    for k, c in enumerate(counters):
        assert got[892 * k: 892 * (k + 1)] == bytes(st.vcdus[c]), k
        assert not want_i[k, 4]
    lines = p.stdout.strip().splitlines()
    assert f"{len(cadu)} frames (" in lines[-2] and "/ 16372" in lines[-2] and "pass.cadu" in lines[-2]      # the --cadu line stays as it is
    m = re.fullmatch(r"(\S+)\.vcdu: (\d+) frames, (\d+) uncorrectable, (\d+) bytes corrected;((?: vcid \d+: \d+ frames, \d+ counter gaps,?)+| no VCID)", lines[-1])
    assert m, lines[-1]
    rep = rs.report(want_v, want_i)
    assert (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (rep.frames, rep.uncorrectable_frames, rep.bytes_corrected)
    per = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"vcid (\d+): (\d+) frames, (\d+) counter gaps", m.group(5))}
    assert per == {v: (rep.frames_per_vcid[v], rep.counter_gaps_per_vcid[v]) for v in rep.frames_per_vcid}
    assert per[5][0] >= 6
    data, rep2 = rs.decode_file(tmp_path / "pass.cadu", device=gpu_device)
    assert data == got and rep2.frames == rep.frames
    alone = subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), "--vcdu", "-o", str(tmp_path / "alone.s"), str(wav)], capture_output=True,
                           text=True, cwd=tmp_path, timeout=300)
    assert alone.returncode == 0 and (tmp_path / "alone.vcdu").read_bytes() == got and not (tmp_path / "alone.cadu").exists()
    assert "alone.vcdu" in alone.stdout.strip().splitlines()[-1] and ".cadu" not in alone.stdout
