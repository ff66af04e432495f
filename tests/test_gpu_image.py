"""GPU tests of the image layer (include/meteor_demod_amd_image.h): both kernels against the host model, byte for byte, on batches
whose neighbouring frames and packets take different paths; guard regions; the entries' argument checks; the pieces of the host
entry; a noisy framed stream from soft symbols to the picture that was sent; and the C host's --image.  Every GPU step runs once;
every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import frames_util as U
import image_util as I

pytestmark = pytest.mark.gpu


def _dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{gpu_device}")


def _stream_handle(gpu_device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)


# ----------------------------------------------------------------------------------------------------- kernels against model
@pytest.mark.parametrize("with_info", [True, False])
@pytest.mark.parametrize("n", [1, 2, 5, 67])
def test_packets_find_equals_the_model(n, with_info, gpu_device):
    """The damaged demux batch (invalid pointer, missing frame, uncorrectable frame, foreign VCID, corrupted length; headers split
    1/5 .. 5/1, packets over 2 and 3 frames), cut to n frames (67 crosses a wave), with and without the reports."""
    from meteor_demod_amd import image
    vcdu, info, meta, want = I.demux_batch(n)
    model = image.model_find(vcdu, info if with_info else None)
    got = image.descriptors(image.find(_dev(vcdu, gpu_device), _dev(info, gpu_device) if with_info else None))
    print(f"n {n}, reports {with_info}: {len(got)} accepted of {sum(1 for m in meta if m[0] < 882 * n)}")
    assert np.array_equal(got, model)
    if with_info:
        assert [(int(d["apid"]), int(d["seq"]), int(d["length"])) for d in got] == want


@pytest.mark.parametrize("m", [1, 2, 65, 130])
def test_image_decode_equals_the_model(m, gpu_device):
    """q 10 / 50 / 100, flat and noisy strips, truncated, corrupt and non-image packets, packets across 2 and 3 frames, side by side in
    the lanes of a wave: strips and reports are the model's, and every clean strip is what the independent decoder gives."""
    from meteor_demod_amd import image
    packets, vcdu, clean = I.decode_batch()
    desc = image.model_find(vcdu)[:m]
    assert [int(d["length"]) for d in desc] == [len(p) for p in packets[:m]]
    want_s, want_i = image.model_decode(vcdu, desc)
    got_s, got_i = image.decode(_dev(vcdu, gpu_device), _dev(desc.view(np.uint8).reshape(-1, 16), gpu_device))
    got_s, got_i = got_s.cpu().numpy(), image.strip_infos(got_i)
    flags = [int(x) for x in got_i["flags"]]
    print(f"m {m}: flags {sorted(set(flags))}, blocks {sorted(set(int(x) for x in got_i['mcus']))}, longest {max(len(p) for p in packets[:m])} bytes")
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
    for k in range(m):
        if clean[k] is not None:
            assert np.array_equal(got_s[k], clean[k]["strip"]) and flags[k] == 0 and int(got_i[k]["bits_used"]) == clean[k]["bits_used"], k
    if m == 130:
        assert {0, I.TRUNCATED, I.NOT_IMAGE} <= set(flags)


# --------------------------------------------------------------------------------------------------------- guard regions
@pytest.mark.parametrize("shift", [0, 4, 1000])
def test_guard_regions(shift, gpu_device):
    """The inputs inside garbage on both sides: the results are those of the inputs alone.  The outputs between canaries: they
    survive.  The inputs are only read."""
    import torch
    from meteor_demod_amd import image
    packets, vcdu, _ = I.decode_batch()
    n = 9
    vcdu = vcdu[:n]
    want_d = image.model_find(vcdu)
    m = len(want_d)
    want_s, want_i = image.model_decode(vcdu, want_d)
    rng = np.random.default_rng(shift)
    buf = rng.integers(0, 256, 4096 + n * 892 + 4096, dtype=np.uint8)
    start = 2048 + shift
    buf[start: start + n * 892] = vcdu.reshape(-1)
    d = _dev(buf, gpu_device)
    pad = 64 + shift % 64
    desc = torch.full((pad + m * 16 + 64,), 0xA5, dtype=torch.uint8, device=d.device)
    total = torch.full((3,), -1, dtype=torch.int64, device=d.device)
    st = _stream_handle(gpu_device)
    assert image.lib().mdemod_packets_find_device(None, C.c_void_p(d.data_ptr() + start), None, n, C.c_void_p(desc.data_ptr() + pad), m,
                                                  C.c_void_p(total.data_ptr() + 8), gpu_device, st) == 0
    strips = torch.full((pad + m * 896 + 64,), 0x5A, dtype=torch.uint8, device=d.device)
    sinfo = torch.full((16 + m * 16 + 16,), 0xC3, dtype=torch.uint8, device=d.device)
    assert image.lib().mdemod_image_decode_device(None, C.c_void_p(d.data_ptr() + start), n, C.c_void_p(desc.data_ptr() + pad), m,
                                                  C.c_void_p(strips.data_ptr() + pad), C.c_void_p(sinfo.data_ptr() + 16), gpu_device, st) == 0
    de, to, ss, si = desc.cpu().numpy(), total.cpu().numpy(), strips.cpu().numpy(), sinfo.cpu().numpy()
    assert (de[:pad] == 0xA5).all() and (de[-64:] == 0xA5).all() and to.tolist() == [-1, m, -1]
    assert (ss[:pad] == 0x5A).all() and (ss[-64:] == 0x5A).all() and (si[:16] == 0xC3).all() and (si[-16:] == 0xC3).all()
    assert np.array_equal(image.descriptors(de[pad:-64]), want_d)
    assert np.array_equal(ss[pad:-64].reshape(m, 8, 112), want_s) and np.array_equal(image.strip_infos(si[16:-16]), want_i)
    assert np.array_equal(d.cpu().numpy(), buf)


# ------------------------------------------------------------------------------------------------------------- arguments
def test_arguments(gpu_device):
    import torch
    from meteor_demod_amd import _capi, image
    lib, st = image.lib(), _stream_handle(gpu_device)
    assert lib.mdemod_packets_find_device(None, None, None, 0, None, 0, None, gpu_device, st) == 0              # n = 0: nothing to do
    assert lib.mdemod_image_decode_device(None, None, 0, None, 0, None, None, gpu_device, st) == 0              # n_desc = 0
    empty = torch.zeros((0, 892), dtype=torch.uint8, device=f"cuda:{gpu_device}")
    assert tuple(image.find(empty).shape) == (0, 16) and tuple(image.decode(empty, image.find(empty))[0].shape) == (0, 8, 112)
    vcdu, info, _, want = I.demux_batch(22)
    n, m = 22, len(want)
    model = image.model_find(vcdu, info)
    size = n * 892 + n * 8 + m * 16 + 8 + m * 896 + m * 16
    buf = torch.zeros(size + 64, dtype=torch.uint8, device=f"cuda:{gpu_device}")
    base = buf.data_ptr()
    assert base % 8 == 0
    a_v, a_i = base, base + n * 892
    a_d, a_t = a_i + n * 8, a_i + n * 8 + m * 16
    a_s, a_r = a_t + 8, a_t + 8 + m * 896
    buf[: n * 892] = _dev(vcdu.reshape(-1), gpu_device)
    buf[n * 892: n * 892 + n * 8] = _dev(info.reshape(-1), gpu_device)

    def find(opts, v, i, d, cap, t):
        return lib.mdemod_packets_find_device(C.byref(opts) if opts is not None else None, C.c_void_p(v), C.c_void_p(i), n, C.c_void_p(d), cap, C.c_void_p(t),
                                              gpu_device, st)

    def decode(opts, v, d, s, r):
        return lib.mdemod_image_decode_device(C.byref(opts) if opts is not None else None, C.c_void_p(v), n, C.c_void_p(d), m, C.c_void_p(s), C.c_void_p(r),
                                              gpu_device, st)

    def refused(word, rc):
        text = _capi.last_error()
        print(f"{word}: rc {rc}, '{text}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in text

    # cap smaller than the total: the total is right, the first cap descriptors are right, nothing behind them is written
    buf[a_d - base: a_t - base] = 0xEE
    assert find(None, a_v, a_i, a_d, 7, a_t) == 0
    host = buf.cpu().numpy()
    assert int(host[a_t - base: a_t - base + 8].view(np.uint64)[0]) == m
    assert np.array_equal(image.descriptors(host[a_d - base: a_d - base + 7 * 16]), model[:7]) and (host[a_d - base + 7 * 16: a_t - base] == 0xEE).all()
    assert find(None, a_v, a_i, a_d, m, a_t) == 0 and decode(None, a_v, a_d, a_s, a_r) == 0
    refused("needed", find(None, 0, a_i, a_d, m, a_t))
    refused("needed", find(None, a_v, a_i, 0, m, a_t))
    refused("needed", find(None, a_v, a_i, a_d, m, 0))
    refused("multiples of 4", find(None, a_v + 2, a_i, a_d, m, a_t))
    refused("multiple of 8", find(None, a_v, a_i, a_d, m, a_t + 4))
    refused("intersect", find(None, a_v, a_i, a_v + 892 * n - 4, m, a_t))
    refused("intersect", find(None, a_v, a_i, a_i, m, a_t))
    refused("intersect", find(None, a_v, a_i, a_d, m, a_d + 16))
    refused("needed", decode(None, 0, a_d, a_s, a_r))
    refused("needed", decode(None, a_v, 0, a_s, a_r))
    refused("needed", decode(None, a_v, a_d, 0, a_r))
    refused("needed", decode(None, a_v, a_d, a_s, 0))
    refused("multiples of 4", decode(None, a_v, a_d, a_s + 1, a_r))
    refused("intersect", decode(None, a_v, a_d, a_v + 4, a_r))
    refused("intersect", decode(None, a_v, a_d, a_d, a_r))
    refused("intersect", decode(None, a_v, a_d, a_s, a_s + 896 * m - 4))
    for word, opts in (("vcid", dict(vcid=64)), ("period", dict(period=0)), ("apid", dict(apids=(63, 65, 66))), ("repeated", dict(apids=(65, 65, 66))),
                       ("piece_frames", dict(piece_frames=(1 << 20) + 1))):
        refused(word, find(image.make_opts(**opts), a_v, a_i, a_d, m, a_t))
        refused(word, decode(image.make_opts(**opts), a_v, a_d, a_s, a_r))
    # a descriptor that points outside the batch is reported in its strip's flags, never followed
    d = model[:3].copy()
    d["start"][1], d["start"][2], d["length"][2] = n * 882 - 10, 0, 70000
    strips, sinfo = image.decode(_dev(vcdu, gpu_device), _dev(d.view(np.uint8).reshape(-1, 16), gpu_device))
    want_s, want_i = image.model_decode(vcdu, d)
    got_i = image.strip_infos(sinfo)
    assert np.array_equal(got_i, want_i) and np.array_equal(strips.cpu().numpy(), want_s) and [int(x) for x in got_i["flags"][1:]] == [I.OUTSIDE, I.OUTSIDE]
    with pytest.raises(_capi.MdemodError) as e:
        image.vcdu_to_image(vcdu, info, vcid=99, device=gpu_device)
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "vcid" in e.value.detail
    torch.cuda.synchronize(gpu_device)


# ---------------------------------------------------------------------------------------------------------------- pieces
def test_host_entry_in_pieces_equals_the_device_path(gpu_device):
    """The picture's frames and the damaged batch through mdemod_image_decode_host in pieces of 1, 3 and 8192 frames: packets,
    strips, placement and pictures are those of find + decode on the whole batch."""
    from meteor_demod_amd import image
    pic, packets, frames = I.sent()
    vcdu, info, _, want = I.demux_batch()
    whole = image.vcdu_to_image(_dev(frames, gpu_device))
    whole_d = image.vcdu_to_image(_dev(vcdu, gpu_device), _dev(info, gpu_device))
    assert len(whole_d.desc) == len(want)
    for piece in (1, 3, 8192):
        for ref, args in ((whole, (frames, None)), (whole_d, (vcdu, info))):
            got = image.vcdu_to_image(*args, piece_frames=piece, device=gpu_device)
            for name in ("desc", "sinfo", "strips", "place"):
                assert np.array_equal(getattr(got, name), getattr(ref, name)), (piece, name)
            assert got.summary == ref.summary and all(np.array_equal(got.images[a], ref.images[a]) and np.array_equal(got.filled[a], ref.filled[a]) for a in ref.images)
    assert np.array_equal(np.stack([whole.images[a] for a in (64, 65, 66)]), I.expected_picture(packets, I.PIC_ROWS))


# --------------------------------------------------------------------------------------------------------------- streams
def test_soft_to_image_gives_the_picture_that_was_sent(gpu_device):
    """The picture's frames at Es/N0 = 3 dB through sync search, tracker, Viterbi, Reed-Solomon, demux and decoder without leaving the
    device before the strips: the three pictures are the sent packets through the independent decoder (that is the sender's
    quantisation loss and nothing else), every cell filled."""
    from meteor_demod_amd import image
    pic, packets, _ = I.sent()
    st = I.stream()
    want = I.expected_picture(packets, I.PIC_ROWS)
    res, found = image.soft_to_image(_dev(st.received(2, 3.0, seed=77), gpu_device))
    loss = int(np.abs(want.astype(int) - pic).max())
    print(f"{len(found)} frames tracked of {st.n_frames}; {res.summary}; the sender's loss at q {I.PIC_Q}: peak {loss} grey levels")
    assert len(found) >= st.n_frames - I.TAIL_IDLE and res.summary["placed"] == 42 and res.summary["truncated"] == 0 and res.summary["rows"] == I.PIC_ROWS
    for k, a in enumerate((64, 65, 66)):
        assert np.array_equal(res.images[a], want[k]) and res.filled[a].all()
    assert res.summary["per_apid"][64] == 14 and sum(1 for d in res.desc if d["apid"] == 70) == 1


# ------------------------------------------------------------------------------------------------------------------- CLI
def _pgm(path):
    raw = path.read_bytes()
    m = re.match(rb"P5\n(\d+) (\d+)\n255\n", raw)
    assert m, raw[:20]
    w, h = int(m.group(1)), int(m.group(2))
    assert len(raw) == m.end() + w * h
    return np.frombuffer(raw[m.end():], dtype=np.uint8).reshape(h, w)


def test_cli_image(tmp_path, gpu_device):
    """--image on the recording of the picture: three PGMs whose pixels are vcdu_to_image of the same frames and the picture that was
    sent, the line, --apids, the refusals; what --cadu --vcdu write and print is the same with and without --image."""
    from conftest import ROOT
    from meteor_demod_amd import image, rs
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    pic, packets, _ = I.sent()
    st, iq = I.recording()
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))

    def run(name, *flags):
        return subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), *flags, "-o", str(tmp_path / name), str(wav)], capture_output=True,
                              text=True, cwd=tmp_path, timeout=300)

    p = run("pass.s", "--cadu", "--vcdu", "--image")
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    cadu = np.frombuffer((tmp_path / "pass.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    assert (tmp_path / "pass.vcdu").read_bytes() == vcdu.tobytes()
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    want = I.expected_picture(packets, I.PIC_ROWS)
    for k, a in enumerate((64, 65, 66)):
        got = _pgm(tmp_path / f"pass_{a}.pgm")
        assert got.shape == (8 * I.PIC_ROWS, 1568) and np.array_equal(got, res.images[a]) and np.array_equal(got, want[k])
    lines = p.stdout.strip().splitlines()
    m = re.fullmatch(r"(\S+)pass: (\d+) packets; image packets apid 64: (\d+), apid 65: (\d+), apid 66: (\d+); (\d+) strips truncated; (\d+) lines; "
                     r"([\d.]+) % of cells filled", lines[-1])
    assert m, lines[-1]
    assert [int(m.group(k)) for k in range(2, 8)] == [len(res.desc), 14, 14, 14, 0, 8 * I.PIC_ROWS] and float(m.group(8)) == 100.0
    # the .vcdu through decode_file: the same pictures, and a report that says what the line says
    res2, rep = image.decode_file(tmp_path / "pass.vcdu", device=gpu_device)
    assert all(np.array_equal(res2.images[a], res.images[a]) for a in (64, 65, 66))
    assert (rep.frames, rep.packets, rep.strips_placed, rep.strips_truncated, rep.strips_dropped, rep.sequence_gaps) == (len(vcdu), len(res.desc), 42, 0, 0, 0)
    assert rep.lines_per_channel == {64: 8, 65: 8, 66: 8} and rep.packets_per_apid[64] == 14 and rep.packets_per_apid[70] == 1 and rep.cells_filled == 42
    # the lines and files of --cadu --vcdu are what they are without --image
    plain = run("plain.s", "--cadu", "--vcdu")
    assert plain.returncode == 0 and (tmp_path / "plain.vcdu").read_bytes() == vcdu.tobytes() and (tmp_path / "plain.cadu").read_bytes() == cadu.tobytes()
    assert [x.replace("plain.", "pass.") for x in plain.stdout.strip().splitlines()] == lines[:-1] and not list(tmp_path.glob("plain*.pgm"))
    # --image alone: the pictures, neither .vcdu nor .cadu; --apids: only channels that received a strip are written
    alone = run("alone.s", "--image", "--apids", "64,65,68")
    assert alone.returncode == 0, alone.stderr
    assert not (tmp_path / "alone.vcdu").exists() and not (tmp_path / "alone.cadu").exists() and not (tmp_path / "alone_68.pgm").exists()
    assert np.array_equal(_pgm(tmp_path / "alone_65.pgm"), want[1]) and np.array_equal(_pgm(tmp_path / "alone_64.pgm"), want[0])
    last = alone.stdout.strip().splitlines()[-1]
    assert "apid 68: 0" in last and "apid 64: 14" in last and ".vcdu" not in alone.stdout and ".cadu" not in alone.stdout
    for flags, word in ((("--apids", "64,65,66"), "only with --image"), (("--image", "--stdout"), "not with --stdout"),
                        (("--image", "--apids", "64,65,70"), "64 .. 69"), (("--image", "--apids", "64,64,66"), "different")):
        r = run("no.s", *flags)
        assert r.returncode == 1 and word in r.stderr and not (tmp_path / "no.s").exists(), (flags, r.stderr)
