"""Rates of the frame layer (include/meteor_demod_amd_frames.h); numbers go to profiles/frames.md.

    python tools/frames_rate.py gpu [--symbols 2^24 2^26 --reps 3] [--no-demod] [--no-model]
        a framed stream of that many soft symbols (128 frames at Es/N0 7 dB, repeated) in device memory:
          candidates   mdemod_frames_candidates_device between two device events (the kernel fr_candidates and nothing else)
          viterbi      mdemod_frames_viterbi_device on the tracker's frame list, host clock around the synchronous call (fr_viterbi,
                       fr_errors, the list's upload, the error counts' download)
          decode       mdemod_frames_decode_device, host clock: all three steps and the CADUs' copy to the host
          demodulate   mdemod_demodulate_recording of a recording of as many symbols (QPSK 72 ksym/s at 288 kS/s, s16, 12 dB), host
                       clock: the step the frame layer follows, in the same run
          model        the host model (mdemod_frames_model_decode) on one core, on the first 2^22 symbols
        Run it under rocprofv3 --kernel-trace --stats (a run of its own, --no-demod --no-model) for the kernels' own times.
    python tools/frames_rate.py threshold [--seeds 3]
        CPU only: the share of windows whose argmax is not the true marker, per Es/N0, from the host model.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SPS = 4


def _n(s: str) -> int:
    return 1 << int(s[2:]) if s.startswith("2^") else int(s)


def _stream(m: int) -> np.ndarray:
    """m soft symbols: 128 frames (marker + random bytes) at 7 dB, the same 2^20 symbols over and over."""
    import frames_util as U
    base = U.Stream(seed=11, n_frames=128, lead=0, tail=0).received(0, 7.0, seed=12)
    return np.ascontiguousarray(np.tile(base, ((m + len(base) - 1) // len(base), 1))[:m])


def _host_timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def _event_timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return ts


def _fig(ts, m):
    return {"seconds": [round(t, 6) for t in ts], "best_seconds": min(ts), "msymbols_per_s": m / min(ts) / 1e6}


def gpu(a) -> dict:
    import ctypes as C
    import torch
    from meteor_demod_amd import DemodConfig, frames, synth
    from meteor_demod_amd._capi import check
    from meteor_demod_amd.recording import demodulate_recording_native
    out = {}
    for m in a.symbols:
        soft = _stream(m)
        d = torch.from_numpy(soft).cuda()
        r = {"symbols": m}
        r["candidates_kernel"] = _fig(_event_timed(lambda: frames.candidates_tensor(d), a.reps), m)
        found = frames.track(frames.candidates(d), m)
        r["frames"] = len(found)
        # the entries themselves, on buffers made once: no Python marshalling inside the timed window
        lib, st, cap = frames.lib(), C.c_void_p(torch.cuda.current_stream(0).cuda_stream), max(1, m // 8192)
        arr, n = frames._to_c(found), C.c_uint64()
        cadu_dev = torch.empty((max(1, len(found)), 1024), dtype=torch.uint8, device=d.device)
        r["viterbi_call"] = _fig(_host_timed(lambda: check(lib.mdemod_frames_viterbi_device(C.c_void_p(d.data_ptr()), m, arr, len(found),
                                                                                          C.c_void_p(cadu_dev.data_ptr()), 0, st), "viterbi"), a.reps), m)
        info, cadu, o = (frames.MdemodFrameInfo * cap)(), np.zeros((cap, 1024), dtype=np.uint8), frames.make_opts()
        r["decode_device_call"] = _fig(_host_timed(lambda: check(lib.mdemod_frames_decode_device(C.byref(o), C.c_void_p(d.data_ptr()), m, cadu.ctypes.data,
                                                                                                info, cap, C.byref(n), 0, st), "decode"), a.reps), m)
        r["channel_errors_mean"] = float(np.mean([f.channel_errors for f in info[: n.value]])) if n.value else 0.0
        del d
        if not a.no_model:
            mm = min(m, 1 << 22)
            t0 = time.perf_counter()
            _, fr = frames.model_decode(soft[:mm])
            r["model_one_core"] = {"symbols": mm, "frames": len(fr), **_fig([time.perf_counter() - t0], mm)}
        if not a.no_demod:
            cfg = DemodConfig(samplerate=72000 * SPS)
            sst = synth.make_stream(7, 72000 * SPS, 72000, f0_hz=300.0, esn0_db=12.0, rms=3000.0, dc=(0.0, 0.0))
            iq = synth.generate_device([sst], m * SPS)[0]
            torch.cuda.synchronize()
            syms = []

            def once():
                s, _ = demodulate_recording_native(cfg, iq)
                syms.append(int(s.shape[0]))
            r["demodulate_recording_call"] = {"samples": m * SPS, **_fig(_host_timed(once, min(a.reps, 2)), m), "symbols_out": syms[-1]}
            del iq
            r["frame_layer_over_demodulation"] = r["decode_device_call"]["best_seconds"] / r["demodulate_recording_call"]["best_seconds"]
        torch.cuda.empty_cache()
        out[str(m)] = r
        print(json.dumps({str(m): r}), flush=True)
    return out


def threshold(a) -> dict:
    import frames_util as U
    from meteor_demod_amd import frames
    res = {}
    for db in (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0):
        miss = total = 0
        low_true, high_false = 1 << 30, 0
        for seed in range(a.seeds):
            st = U.Stream(seed=50 + seed, n_frames=32, lead=777, tail=300)
            for h in (0, 3, 5):
                soft = st.received(h, db, seed=1000 * seed + h)
                c = frames.model_candidates(soft)[:32]
                for k, x in enumerate(c):
                    ok = x.position == st.positions[k] and x.hypothesis == h
                    miss += not ok
                    total += 1
                    if ok:
                        low_true = min(low_true, x.score)
                    else:
                        high_false = max(high_false, x.score)
        res[str(db)] = {"windows": total, "missed": miss, "lowest_true_score_that_won": low_true, "highest_false_score_that_won": high_false}
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["gpu", "threshold"])
    ap.add_argument("--symbols", type=_n, nargs="+", default=[1 << 24, 1 << 26])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--no-demod", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", type=Path, help="also write the JSON here")
    a = ap.parse_args()
    if a.what == "gpu":
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: nothing here is measured on the CPU")
    r = {"gpu": gpu, "threshold": threshold}[a.what](a)
    line = json.dumps({a.what: r})
    print(line, flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
