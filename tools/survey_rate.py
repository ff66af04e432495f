"""Rates of the survey (include/meteor_demod_amd_survey.h); numbers go to profiles/survey.md.

    python tools/survey_rate.py kernel [--samples 2^30 --fft 4096 --reps 3]
        the spectrum of 2^30 s16 samples (one recording, rows = 8) through mdemod_spectrum_device, `reps` times, then the front
        end's filter (64 streams x samples / 64, / 8) on the same bytes for scale.  Run it under rocprofv3 --kernel-trace --stats
        (a run of its own) for the kernel times; the host-timed rates it prints include the call's allocations and its
        synchronisation and are only a check.
    python tools/survey_rate.py cli [--samples 2^26]
        one 2.4 MS/s s16 WAV file, LRPT at +301.2 kHz: wall time of the CLI with --offset auto --decimate 8 against
        --offset 301200 --decimate 8, exact and --tiled: what the survey adds.

Bytes per input sample the spectrum must move at least: bps / 4 (read), against the 8 TB/s of HBM.
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
FS = 2400000


def _n(s: str) -> int:
    return 1 << int(s[2:]) if s.startswith("2^") else int(s)


def _recording(n: int):
    """LRPT at +301.2 kHz, 2.4 MS/s s16; beyond 2^24 samples the same 2^24 over and over (the kernels do not care)."""
    import torch
    from meteor_demod_amd import synth
    base = min(n, 1 << 24)
    st = synth.make_stream(7, FS, 72000, f0_hz=301200.0, esn0_db=15.0, rms=3000.0, dc=(0.0, 0.0))
    x = synth.generate_device([st], base)[0]
    if n > base:
        x = x.repeat((n + base - 1) // base, 1)[:n].contiguous()
    torch.cuda.synchronize()
    return x


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def kernel(a) -> dict:
    import ctypes as C
    import torch
    from meteor_demod_amd import DemodConfig, FrontEnd, FrontEndConfig, survey
    from meteor_demod_amd._capi import check
    cfg = DemodConfig(samplerate=FS)
    x = _recording(a.samples)
    out = {"samples": a.samples, "format": "s16", "rows": 8, "reps": a.reps}
    for nfft in a.fft:
        dt = _timed(lambda: survey.spectrum(cfg, x, fft_size=nfft, rows=8), a.reps)
        out[f"spectrum_{nfft}"] = {"seconds_per_call_host_timed": dt, "gsamples_per_s": a.samples / dt / 1e9,
                                   "fraction_of_8TBps": a.samples * 4 / dt / HBM_BYTES_PER_S}
    streams, d = 64, 8
    per = a.samples // streams
    with FrontEnd(cfg, FrontEndConfig(301200.0, d), streams) as f:
        n, off, cnt = f._uniform_rows(x[: per * streams].reshape(streams, per, 2))
        cap = f.max_outputs(n)
        bb = torch.empty((streams, cap, 2), dtype=torch.float32, device=x.device)
        n_out = torch.empty((streams,), dtype=torch.int32, device=x.device)

        def once():
            check(f._lib.mdemod_fe_baseband_device(f._h, C.c_void_p(x.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                   C.c_void_p(bb.data_ptr()), cap, cap, C.c_void_p(n_out.data_ptr()), f._stream()),
                  "mdemod_fe_baseband_device")
        dt = _timed(once, a.reps)
    out["fe_filter_div8_same_bytes"] = {"seconds_per_call_host_timed": dt, "gsamples_per_s": per * streams / dt / 1e9,
                                        "fraction_of_8TBps": per * streams * (4 + 8 / d) / dt / HBM_BYTES_PER_S}
    return out


def cli(a) -> dict:
    import torch
    exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    x = _recording(a.samples).cpu().numpy()
    res = {"samples": a.samples, "samplerate": FS}
    with tempfile.TemporaryDirectory() as td:
        wav = Path(td) / "rec.wav"
        data = x.tobytes()
        wav.write_bytes(b"RIFF" + struct.pack("<I", (36 + len(data)) & 0xFFFFFFFF) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, FS, FS * 4, 4, 16)
                        + b"data" + struct.pack("<I", len(data) & 0xFFFFFFFF) + data)
        del data
        for mode, flags in (("exact", []), ("tiled", ["--tiled"])):
            for name, extra in (("offset_given", ["--offset", "301200"]), ("offset_auto", ["--offset", "auto"])):
                best = None
                for _ in range(2):
                    t0 = time.perf_counter()
                    p = subprocess.run([str(exe), "-q", "-B", *flags, "-o", str(Path(td) / "out.s"), *extra, "--decimate", "8", str(wav)],
                                       capture_output=True, text=True)
                    dt = time.perf_counter() - t0
                    if p.returncode:
                        raise RuntimeError(p.stderr)
                    best = dt if best is None else min(best, dt)
                res[f"{mode}_{name}"] = {"wall_seconds_best_of_2": best}
            g, s = res[f"{mode}_offset_given"]["wall_seconds_best_of_2"], res[f"{mode}_offset_auto"]["wall_seconds_best_of_2"]
            res[f"{mode}_survey_adds"] = {"seconds": s - g, "ratio": s / g}
    torch.cuda.synchronize()
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "cli"])
    ap.add_argument("--samples", type=_n)
    ap.add_argument("--fft", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=Path, help="also write the JSON here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured on the CPU")
    a.samples = a.samples or {"kernel": 1 << 30, "cli": 1 << 26}[a.what]
    r = {"kernel": kernel, "cli": cli}[a.what](a)
    line = json.dumps({a.what: r})
    print(line, flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
