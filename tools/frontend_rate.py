"""Rates of the front end (include/meteor_demod_amd_frontend.h); numbers go to profiles/frontend.md.

    python tools/frontend_rate.py kernel [--streams 64 --samples 2^24 --reps 5]
        64 streams x 2^24 s16 samples at 2.4 MS/s / 8 through mdemod_fe_baseband_device, `reps` times.  Run it under
        rocprofv3 --kernel-trace --stats (a run of its own) for the kernel time; the host-timed rate it prints is only a check.
    python tools/frontend_rate.py e2e [--streams 16384 --samples 2^16]
        front end + demodulator (mdemod_fe_process_device, 2.048 MS/s / 8, -f 64 -O 4 behind it) against the direct path
        (mdemod_process_device_uniform at 2.048 MS/s, -f 64 -O 4) on the same s16 input: input samples per second, device-timed.
    python tools/frontend_rate.py cli [--samples 2^24]
        one 2.4 MS/s s16 WAV file in exact mode, wall time of the CLI with and without --offset 300k --decimate 8.

Bytes per input sample the front end must move at least: bps / 4 (read) + 8 / D (f32 I, Q written), against the 8 TB/s of HBM.
"""
from __future__ import annotations

import argparse
import json
import struct
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8.0e12


def _n(s: str) -> int:
    return 1 << int(s[2:]) if s.startswith("2^") else int(s)


def _signal(streams: int, n: int, fs: int, offset: float):
    import torch
    from meteor_demod_amd import synth
    recs = [synth.make_stream(100 + i, fs, 72000, f0_hz=offset + 37.0 * i) for i in range(min(streams, 64))]
    x = synth.generate_device(recs, n)
    if streams > len(recs):                                       # (more streams than distinct recordings: repeat them)
        x = x.repeat((streams + len(recs) - 1) // len(recs), 1, 1)[:streams].contiguous()
    torch.cuda.synchronize()
    return x


def kernel(a) -> dict:
    import ctypes as C
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig
    fs, d = 2400000, 8
    x = _signal(a.streams, a.samples, fs, 300000.0)
    with FrontEnd(DemodConfig(samplerate=fs), FrontEndConfig(300000.0, d), a.streams) as f:
        n, off, cnt = f._uniform_rows(x)
        flat = x.reshape(-1, 2)
        cap = f.max_outputs(n)
        bb = torch.empty((a.streams, cap, 2), dtype=torch.float32, device=x.device)
        n_out = torch.empty((a.streams,), dtype=torch.int32, device=x.device)

        def once():
            from meteor_demod_amd._capi import check
            check(f._lib.mdemod_fe_baseband_device(f._h, C.c_void_p(flat.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                   C.c_void_p(bb.data_ptr()), cap, cap, C.c_void_p(n_out.data_ptr()), f._stream()),
                  "mdemod_fe_baseband_device")
        once()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            once()
        e1.record()
        torch.cuda.synchronize()
        dt = e0.elapsed_time(e1) / 1e3 / a.reps
    samples = a.streams * a.samples
    per_sample = 16 / 4 + 8 / d
    return {"what": "front end only (fe_filter + fe_advance), device events around the calls", "streams": a.streams,
            "samples_per_stream": a.samples, "decimation": d, "seconds_per_call": dt, "gsamples_per_s": samples / dt / 1e9,
            "bytes_per_input_sample": per_sample, "fraction_of_8TBps": samples * per_sample / dt / HBM_BYTES_PER_S}


def e2e(a) -> dict:
    import torch
    from meteor_demod_amd import DemodConfig, Demodulator, FrontEnd, FrontEndConfig
    fs, d = 2048000, 8
    cfg = DemodConfig(samplerate=fs, rrc_order=64, interp_factor=4)
    x = _signal(a.streams, a.samples, fs, 300000.0)
    samples = a.streams * a.samples
    out = {"streams": a.streams, "samples_per_stream": a.samples, "config": "QPSK 72k, -f 64 -O 4, s16 input at 2.048 MS/s"}

    def timed(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3 / reps
    with Demodulator(cfg, a.streams) as dm:
        soft = torch.empty((a.streams, dm.max_symbols(a.samples), 2), dtype=torch.int8, device=x.device)
        dt = timed(lambda: dm.process(x, soft=soft))
        out["direct"] = {"kernel": dm.kernel_name, "seconds_per_call": dt, "gsamples_per_s": samples / dt / 1e9}
    del soft
    with FrontEnd(cfg, FrontEndConfig(300000.0, d), a.streams) as f:
        soft = torch.empty((a.streams, f.max_symbols(a.samples), 2), dtype=torch.int8, device=x.device)
        dt = timed(lambda: f.process(x, soft=soft))
        out["front_end_div8"] = {"kernel": f.kernel_name, "seconds_per_call": dt, "gsamples_per_s": samples / dt / 1e9}
    out["speedup"] = out["front_end_div8"]["gsamples_per_s"] / out["direct"]["gsamples_per_s"]
    return out


def cli(a) -> dict:
    import numpy as np
    import torch
    exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    fs = 2400000
    x = _signal(1, a.samples, fs, 300000.0)[0].cpu().numpy()
    res = {"samples": a.samples, "samplerate": fs}
    with tempfile.TemporaryDirectory() as td:
        wav = Path(td) / "rec.wav"
        data = x.astype(np.int16).tobytes()
        wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, fs, fs * 4, 4, 16)
                        + b"data" + struct.pack("<I", len(data)) + data)
        for name, extra in (("direct", []), ("offset_300k_decimate_8", ["--offset", "300k", "--decimate", "8"])):
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                p = subprocess.run([str(exe), "-q", "-B", "-o", str(Path(td) / "out.s"), *extra, str(wav)], capture_output=True, text=True)
                dt = time.perf_counter() - t0
                if p.returncode:
                    raise RuntimeError(p.stderr)
                best = dt if best is None else min(best, dt)
            res[name] = {"wall_seconds": best, "msamples_per_s": a.samples / best / 1e6}
    torch.cuda.synchronize()
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "e2e", "cli"])
    ap.add_argument("--streams", type=int)
    ap.add_argument("--samples", type=_n)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=Path, help="also write the JSON here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured on the CPU")
    defaults = {"kernel": (64, 1 << 24), "e2e": (16384, 1 << 16), "cli": (1, 1 << 24)}[a.what]
    a.streams = a.streams or defaults[0]
    a.samples = a.samples or defaults[1]
    r = {"kernel": kernel, "e2e": e2e, "cli": cli}[a.what](a)
    line = json.dumps({a.what: r})
    print(line, flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
