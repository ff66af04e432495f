"""GPU tests of the front end (include/meteor_demod_amd_frontend.h): the baseband against a float64 model, its independence of
call sizes and batch slots, the demodulator on it (the reference's own bytes where the front end is the identity, the oracle
on the baseband elsewhere), the capability it adds (an off-centre signal in a wide recording next to an interferer), the tiled
path and the CLI."""
from __future__ import annotations

import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_npz

pytestmark = pytest.mark.gpu

CLI = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
_NP = {8: np.uint8, 16: np.int16, 32: np.float32}


def _torch_dtype(bps):
    import torch
    return {8: torch.uint8, 16: torch.int16, 32: torch.float32}[bps]


def _model(x: np.ndarray, bps: int, fs: int, d: int, offset: float, h: np.ndarray, n0: int = 0) -> np.ndarray:
    """float64 model: the library's phase words (full 32 bits), the library's float taps, zero history."""
    from meteor_demod_amd.frontend import phase_step
    xc = x.astype(np.float64)
    if bps == 8:
        xc = xc - 128.0
    z = xc[:, 0] + 1j * xc[:, 1]
    step = phase_step(offset, fs)
    if step:
        n = np.arange(n0, n0 + len(z), dtype=np.uint64)
        p = (n * np.uint64(step)) & np.uint64(0xFFFFFFFF)
        z = z * np.exp(2j * np.pi * p.astype(np.float64) / 2.0 ** 32)
    y = np.convolve(z, h.astype(np.float64))[: len(z)]
    return y[::d]


def _input(bps, n, seed):
    rng = np.random.default_rng(seed)
    if bps == 8:
        return rng.integers(0, 256, size=(n, 2)).astype(np.uint8)
    if bps == 16:
        return np.clip(rng.normal(0, 3000, size=(n, 2)), -32768, 32767).astype(np.int16)
    return rng.normal(0, 0.3, size=(n, 2)).astype(np.float32)


def _rms(x, bps):
    xc = x.astype(np.float64) - (128.0 if bps == 8 else 0.0)
    return float(np.sqrt((xc ** 2).sum(axis=1).mean()))


@pytest.mark.parametrize("bps", [8, 16, 32])
def test_baseband_matches_float64_model(bps, gpu_device):
    """u8 / s16 / f32 x D in {1, 2, 5, 8, 13, 40, 128} (fs = D x 250 kS/s) x offsets {0, +312.5 kHz, -0.37 fs}: max |error| <= 1e-4
    of the input's RMS, and exactly ceil(n / D) outputs."""
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig, design_taps
    for d in (1, 2, 5, 8, 13, 40, 128):
        fs = 250000 * d
        n = max(40000, 260 * d) + 3
        x = _input(bps, n, seed=d * 10 + bps)
        rms = _rms(x, bps)
        for off in (0.0, 312500.0, -0.37 * fs):
            if abs(off) >= fs / 2:
                continue
            cfg = DemodConfig(samplerate=fs, bps=bps)
            fe = FrontEndConfig(off, d)
            h, _ = design_taps(cfg, fe)
            with FrontEnd(cfg, fe, 1) as f:
                bb, cnt = f.baseband(torch.from_numpy(x).to(f"cuda:{gpu_device}").reshape(1, n, 2))
            got = bb[0, : int(cnt[0])].cpu().numpy().astype(np.float64)
            want = _model(x, bps, fs, d, off, h)
            assert int(cnt[0]) == -(-n // d) == len(want)
            err = np.abs((got[:, 0] + 1j * got[:, 1]) - want).max()
            assert err <= 1e-4 * rms, (bps, d, off, err / rms)
            if off == 0.0 and d == 1:
                assert np.array_equal(got.astype(np.float32), x.astype(np.float32) - (128 if bps == 8 else 0))


def _lrpt(n, fs=2400000, seed=5, offset=301200.0, interferer=-300000.0, rms=6000.0, esn0_db=15.0, oqpsk=False, symrate=72000):
    """A 2.4 MS/s s16 recording on the device: LRPT at `offset` (+ an equal-RMS, near-noiseless LRPT interferer at
    `interferer`, which an unfiltered /8 decimation folds onto it).  Returns (iq [n, 2] int16 device tensor, signal stream)."""
    import torch
    from meteor_demod_amd import synth
    sig = synth.make_stream(seed, fs, symrate, f0_hz=offset, esn0_db=esn0_db, rms=rms, dc=(0.0, 0.0), oqpsk=oqpsk)
    x = synth.generate_device([sig], n)[0].to(torch.int32)
    if interferer is not None:
        jam = synth.make_stream(seed + 1000, fs, symrate, f0_hz=interferer, esn0_db=60.0, rms=rms, dc=(0.0, 0.0), oqpsk=oqpsk)
        x = x + synth.generate_device([jam], n)[0].to(torch.int32)
    return x.clamp(-32768, 32767).to(torch.int16).contiguous(), sig


def test_chunking_does_not_change_a_byte(gpu_device):
    """Random call sizes (1, D-1, D, D+1, primes, 2^16) give the baseband bytes of one call, and the same soft symbols and lock
    events through the demodulator."""
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig
    cfg = DemodConfig(samplerate=2400000)
    fe = FrontEndConfig(300000.0, 8)
    n = 1 << 20
    x, _ = _lrpt(n, offset=300000.0)                          # (no residual: the PLL locks within the first 0.1 s)
    with FrontEnd(cfg, fe, 1) as f:
        whole, cnt = f.baseband(x.reshape(1, n, 2))
        whole = whole[0, : int(cnt[0])].cpu().numpy()
    sizes = [1, 7, 8, 9, 13, 65521, 1 << 16, 3, 8191, 101]
    rng = np.random.default_rng(3)
    parts, at = [], 0
    with FrontEnd(cfg, fe, 1) as f:
        while at < n:
            k = min(int(sizes[rng.integers(len(sizes))]), n - at)
            bb, c = f.baseband(x[at: at + k].reshape(1, k, 2))
            parts.append(bb[0, : int(c[0])].cpu().numpy())
            at += k
    got = np.concatenate(parts)
    assert got.shape == whole.shape and got.tobytes() == whole.tobytes()

    def run(chunks):
        soft, events = [], []
        with FrontEnd(cfg, fe, 1) as f:
            at = 0
            for k in chunks:
                out = f.process(x[at: at + k].reshape(1, k, 2))
                torch.cuda.synchronize()
                soft.append(out[0, : f.status()[0].symbols_this_call].cpu().numpy())
                events += f.lock_events(0)                  # (the transitions of each call)
                at += k
            return np.concatenate(soft), events, f.status()[0].first_lock_symbol
    one = run([n])
    ks, at = [], 0
    while at < n:
        k = min(int(sizes[rng.integers(len(sizes))]) if len(ks) % 3 else 1 << 16, n - at)
        ks.append(k)
        at += k
    many = run(ks)
    assert one[2] >= 0, "the test signal must lock"
    assert one[0].tobytes() == many[0].tobytes() and one[1] == many[1] and one[2] == many[2]


def test_batch_of_70_ragged_streams_equals_each_alone(gpu_device):
    """70 streams (across a wave boundary), ragged counts, two of them reading the same input at different offsets: each
    stream's baseband bytes equal that stream run alone, and its soft symbols too (checked on a few)."""
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig
    cfg = DemodConfig(samplerate=2400000)
    ns = 70
    rng = np.random.default_rng(9)
    counts = [int(rng.integers(0, 200000)) for _ in range(ns)]
    counts[5] = 0
    counts[1] = counts[0] = 180000
    x, _ = _lrpt(sum(counts) + 1)
    offs = np.cumsum([0] + counts[:-1]).astype(np.int64)
    offs[1] = offs[0]                                        # streams 0 and 1: the same samples, two channels
    offsets_hz = [float(v) for v in rng.uniform(-500000, 500000, size=ns)]
    offsets_hz[0], offsets_hz[1] = 300000.0, -300000.0
    dev = f"cuda:{gpu_device}"
    off_t = torch.tensor(offs, dtype=torch.int64, device=dev)
    cnt_t = torch.tensor(counts, dtype=torch.int32, device=dev)
    with FrontEnd(cfg, FrontEndConfig(0.0, 8), ns, offsets=offsets_hz) as f:
        bb, n_out = f.baseband_ragged(x, off_t, cnt_t, max(counts))
        torch.cuda.synchronize()
        bb, n_out = bb.cpu().numpy(), n_out.cpu().numpy()
    with FrontEnd(cfg, FrontEndConfig(0.0, 8), ns, offsets=offsets_hz) as f:
        soft = f.process_ragged(x, off_t, cnt_t, max(counts))
        torch.cuda.synchronize()
        st = f.status()
        soft = soft.cpu().numpy()
    for s in range(ns):
        seg = x[int(offs[s]): int(offs[s]) + counts[s]]
        with FrontEnd(cfg, FrontEndConfig(offsets_hz[s], 8), 1) as f1:
            b1, c1 = f1.baseband(seg.reshape(1, counts[s], 2))
            assert int(n_out[s]) == int(c1[0]) == -(-counts[s] // 8)
            assert bb[s, : n_out[s]].tobytes() == b1[0, : int(c1[0])].cpu().numpy().tobytes(), s
        if s in (0, 1, 5, 63, 64, 69):
            with FrontEnd(cfg, FrontEndConfig(offsets_hz[s], 8), 1) as f1:
                o1 = f1.process(seg.reshape(1, counts[s], 2))
                torch.cuda.synchronize()
                m1 = f1.status()[0].symbols_this_call
                assert st[s].symbols_this_call == m1
                assert soft[s, :m1].tobytes() == o1[0, :m1].cpu().numpy().tobytes(), s
    assert bb[0, : n_out[0]].tobytes() != bb[1, : n_out[1]].tobytes()


@pytest.mark.parametrize("name", ["c1_short", "c3_short", "u8_short", "f32_short"])
def test_identity_front_end_gives_the_references_bytes(name, manifest, gpu_device):
    """D = 1, offset 0: the front end passes the converted samples through, and the demodulator on them (f32) writes the
    reference's own soft symbols (the golden `soft`)."""
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig
    g = load_npz(name)
    cfg = DemodConfig(**manifest["cases"][name]["cfg"])
    x = torch.from_numpy(np.ascontiguousarray(g["input"])).to(f"cuda:{gpu_device}")
    with FrontEnd(cfg, FrontEndConfig(0.0, 1), 1) as f:
        soft = f.process(x.reshape(1, -1, 2))
        torch.cuda.synchronize()
        m = f.status()[0].symbols_this_call
        got = soft[0, :m].cpu().numpy()
    assert got.tobytes() == g["soft"].tobytes()


@pytest.mark.parametrize("oqpsk,symrate", [(False, 72000), (True, 80000)])
def test_demodulator_on_the_baseband_is_the_oracle(oqpsk, symrate, gpu_device):
    """Front-end soft symbols = oracle_py.oracle_demod on the front end's own baseband (fetched to the host), samplerate fs / D,
    f32: the composition is exact.  2.4 MS/s / 8."""
    import torch
    import oracle_py as O
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig
    from meteor_demod_amd.frontend import output_config
    cfg = DemodConfig(samplerate=2400000, symrate=symrate, oqpsk=oqpsk)
    fe = FrontEndConfig(301000.0, 8)
    n = 1 << 21
    x, _ = _lrpt(n, oqpsk=oqpsk, symrate=symrate, interferer=None)
    with FrontEnd(cfg, fe, 1) as f:
        bb, c = f.baseband(x.reshape(1, n, 2))
        base = bb[0, : int(c[0])].cpu().numpy().astype(np.float32)
    with FrontEnd(cfg, fe, 1) as f:
        soft = f.process(x.reshape(1, n, 2))
        torch.cuda.synchronize()
        m = f.status()[0].symbols_this_call
        got = soft[0, :m].cpu().numpy()
    want = O.oracle_demod(output_config(cfg, fe), base)[0]
    assert got.tobytes() == want.tobytes()


def test_off_centre_signal_next_to_an_interferer(gpu_device):
    """2.4 MS/s s16: LRPT at +300 kHz (+1.2 kHz residual), an equal-RMS near-noiseless interferer at -300 kHz (a plain /8
    without the filter folds it exactly onto the signal).  FrontEnd(300 kHz, /8) locks and demodulates it (rail error rate
    < 1e-4, no pairing change, no unresolved block); the demodulator on the raw recording resolves no block."""
    import torch
    from meteor_demod_amd import DemodConfig, Demodulator, FrontEnd, FrontEndConfig, synth
    cfg = DemodConfig(samplerate=2400000)
    n = 1 << 24
    x, sig = _lrpt(n)
    with FrontEnd(cfg, FrontEndConfig(300000.0, 8), 1) as f:
        soft = f.process(x.reshape(1, n, 2))
        torch.cuda.synchronize()
        st = f.status()[0]
        assert st.locked_once and 0 <= st.first_lock_symbol < st.symbols_this_call // 4
        out = soft[0, : st.symbols_this_call].contiguous()
        tc = synth.truth_check(sig, out, first_symbol=int(st.first_lock_symbol) + 20000)
    assert tc["symbols_compared"] > 250000, tc
    assert tc["rail_error_rate"] < 1e-4 and tc["pairing_changes"] == 0 and tc["unresolved_blocks"] == 0, tc
    with Demodulator(cfg, 1) as d:
        raw = d.process(x.reshape(1, n, 2))
        torch.cuda.synchronize()
        m = d.status()[0].symbols_this_call
        tr = synth.truth_check(sig, raw[0, :m].contiguous())
    assert tr["symbols_compared"] == 0, tr


def test_tiled_front_end_is_the_tiled_demodulator_on_the_baseband(gpu_device):
    """demodulate_recording_frontend on 2^26 input samples = demodulate_recording_native(cfg / 8, the baseband) byte for byte,
    = the C entry behind the CLI's --tiled (mdemod_fe_demodulate_recording_host), and passes the truth check."""
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig, demodulate_recording_frontend, synth
    from meteor_demod_amd.frontend import demodulate_recording_frontend_host, output_config
    from meteor_demod_amd.recording import demodulate_recording_native
    cfg = DemodConfig(samplerate=2400000)
    fe = FrontEndConfig(300000.0, 8)
    n = 1 << 26
    x, sig = _lrpt(n, seed=21)
    soft, rep = demodulate_recording_frontend(cfg, fe, x)
    with FrontEnd(cfg, fe, 1) as f:
        bb, c = f.baseband(x.reshape(1, n, 2))
        base = bb[0, : int(c[0])].contiguous()
    soft2, rep2 = demodulate_recording_native(output_config(cfg, fe), base)
    del base, bb
    assert rep.n_symbols == rep2.n_symbols and soft.cpu().numpy().tobytes() == soft2.cpu().numpy().tobytes()
    host_soft, rep3 = demodulate_recording_frontend_host(cfg, fe, x.cpu().numpy())
    assert rep3.n_symbols == rep.n_symbols and host_soft.tobytes() == soft.cpu().numpy().tobytes()
    tc = synth.truth_check(sig, soft.contiguous(), first_symbol=int(rep.first_lock_symbol) + 20000)
    assert tc["rail_error_rate"] < 1e-4 and tc["pairing_changes"] == 0 and tc["unresolved_blocks"] == 0, tc


def _wav(path, fs, bps, data: bytes):
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1 if bps != 32 else 3, 2, fs,
                                                                                    fs * 2 * bps // 8, 2 * bps // 8, bps)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(data)) + data)


def test_cli_front_end(tmp_path, gpu_device):
    """--offset 300k --decimate 8 on a 2.4 MS/s WAV = the unchanged CLI on the front end's baseband saved as raw f32
    (-s 300000 --bps 32); the same with --tiled, and for a batch of three files; --decimate 7 and 16 are refused (exit 1,
    no output file)."""
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig
    cfg = DemodConfig(samplerate=2400000)
    fe = FrontEndConfig(300000.0, 8)
    n = 1 << 21                                      # whole 32 KiB reads of the WAV and of the baseband file
    wavs, raws = [], []
    for k in range(3):
        x, _ = _lrpt(n, seed=40 + k, offset=300000.0)
        w = tmp_path / f"rec{k}.wav"
        _wav(w, 2400000, 16, x.cpu().numpy().tobytes())
        with FrontEnd(cfg, fe, 1) as f:
            bb, c = f.baseband(x.reshape(1, n, 2))
            r = tmp_path / f"bb{k}.raw"
            r.write_bytes(bb[0, : int(c[0])].cpu().numpy().tobytes())
        wavs.append(w)
        raws.append(r)

    def cli(*args):
        p = subprocess.run([str(CLI), "-q", "-B", *map(str, args)], capture_output=True, text=True, cwd=tmp_path, timeout=600)
        return p

    for mode in ([], ["--tiled"]):
        a, b = tmp_path / "a.s", tmp_path / "b.s"
        p = cli(*mode, "--offset", "300k", "--decimate", "8", "-o", a, wavs[0])
        assert p.returncode == 0, p.stderr
        p = cli(*mode, "-s", "300000", "--bps", "32", "-o", b, raws[0])
        assert p.returncode == 0, p.stderr
        assert a.stat().st_size > 100000 and a.read_bytes() == b.read_bytes(), mode
    p = cli("--offset", "300k", "--decimate", "8", *wavs)
    assert p.returncode == 0, p.stderr
    for k in range(3):
        p = cli("-s", "300000", "--bps", "32", "-o", tmp_path / f"one{k}.s", raws[k])
        assert p.returncode == 0, p.stderr
        assert (tmp_path / f"rec{k}.wav.s").read_bytes() == (tmp_path / f"one{k}.s").read_bytes(), k
    for d in ("7", "16"):
        out = tmp_path / f"refused{d}.s"
        p = cli("--decimate", d, "-o", out, wavs[0])
        assert p.returncode == 1 and "decimation" in p.stderr, p.stderr
        assert not out.exists()
