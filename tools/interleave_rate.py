"""Measurements of the 80 k interleaved mode (include/meteor_demod_amd_interleave.h); numbers go to profiles/interleave.md.

    python tools/interleave_rate.py gpu [--symbols 2^26 --reps 3]
        one interleaved stream of that many raw soft symbols (M = 2048, H = 9, Es/N0 7 dB; 16 384 periods repeated) in device
        memory, one process, warm-up and repeats inside it:
          candidates    mdemod_il_candidates_device between two device events
          deinterleave  mdemod_il_deinterleave_device (one segment: the asynchronous path) between two device events, and with a
                        table of 40 segments (the table in device memory; host clock around the synchronous call)
          decode        mdemod_il_decode_device, all three steps, host clock
          viterbi       mdemod_frames_viterbi_device on the resulting stream (a frame every 8192 symbols), host clock around the
                        synchronous call: the step this layer is in front of, and the bar for the gather
    python tools/interleave_rate.py threshold [--seeds 3]
        the share of windows whose candidate is not the sender's (phase, H), per Es/N0, for the 24-way search (host model: its
        bytes are the kernel's)
    python tools/interleave_rate.py model [--symbols 2^22]
        the host model's rate on one core: mdemod_il_model_candidates and mdemod_il_model_deinterleave
    python tools/interleave_rate.py all      the three in one run
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
sys.path.insert(0, str(ROOT / "tools"))

from frames_rate import _event_timed, _fig, _host_timed, _n  # noqa: E402


def _stream(m: int, M: int = 2048) -> np.ndarray:
    """m raw soft symbols: 16 384 interleaved periods through the inverse of H = 9 at 7 dB, over and over (the sync words stay in
    phase: the base is a whole number of periods)."""
    import interleave_util as IU
    snd = IU.Sender(np.random.default_rng(21).integers(0, 2, 72 * 16384, dtype=np.uint8), M, 0, 22, tail=0)
    base = snd.received(9, 7.0, seed=23)
    return np.ascontiguousarray(np.tile(base, ((m + len(base) - 1) // len(base), 1))[:m])


def gpu(a) -> dict:
    import ctypes as C
    import torch
    from meteor_demod_amd import frames, interleave as il
    from meteor_demod_amd._capi import check
    out = {}
    for m in a.symbols:
        d = torch.from_numpy(_stream(m)).cuda()
        r = {"symbols": m, "branch_delay": 2048}
        r["candidates"] = _fig(_event_timed(lambda: il.candidates_tensor(d), a.reps), m)
        segs, P = il.track(il.candidates(d), m)
        r["segments"], r["periods"] = len(segs), P
        lib, st = il.lib(), C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        o = il.make_opts()
        deint = torch.empty((36 * P, 2), dtype=torch.int8, device=d.device)

        def gather(table):
            arr = il._segs_to_c(table)
            return lambda: check(lib.mdemod_il_deinterleave_device(C.byref(o), C.c_void_p(d.data_ptr()), m, arr, len(table), P, C.c_void_p(deint.data_ptr()), 0, st),
                                 "deinterleave")
        many = [il.Segment(0, 40 * (P // 40) * i, (P // 40) * i, 0, 9) for i in range(40)]
        r["deinterleave_40_segments"] = _fig(_host_timed(gather(many), a.reps), m)
        r["deinterleave"] = _fig(_event_timed(gather(segs), a.reps), m)
        r["decode_call"] = _fig(_host_timed(lambda: il.decode(d), a.reps), m)
        found = [frames.Frame(8192 * k, 0, 0, 0, 0, 0) for k in range(36 * P // 8192)]
        arr = frames._to_c(found)
        cadu = torch.empty((max(1, len(found)), 1024), dtype=torch.uint8, device=d.device)
        r["frames"] = len(found)
        r["viterbi"] = _fig(_host_timed(lambda: check(frames.lib().mdemod_frames_viterbi_device(C.c_void_p(deint.data_ptr()), 36 * P, arr, len(found),
                                                                                             C.c_void_p(cadu.data_ptr()), 0, st), "viterbi"), a.reps), m)
        for k in ("candidates", "deinterleave", "deinterleave_40_segments"):
            r[f"{k}_over_viterbi"] = r[k]["best_seconds"] / r["viterbi"]["best_seconds"]
        del d, deint
        torch.cuda.empty_cache()
        out[str(m)] = r
        print(json.dumps({str(m): r}), flush=True)
    return out


def threshold(a) -> dict:
    import interleave_util as IU
    from meteor_demod_amd import interleave as il
    res = {}
    for db in (-14.0, -12.0, -10.0, -8.0, -6.0, -4.0, -2.0, 0.0, 3.0):
        miss = total = 0
        low_true, high_false = 1 << 30, 0
        for seed in range(a.seeds):
            snd = IU.random_sender(300 + seed, 32 * 64, 2, lead=(13 * seed + 5) % 40)
            for H in (0, 11, 21):
                soft = snd.received(H, db, seed=1000 * seed + H)
                for w, c in enumerate(il.model_candidates(soft)[:32]):
                    ok = c.position - 2560 * w == snd.lead and c.hypothesis == H
                    miss += not ok
                    total += 1
                    if ok:
                        low_true = min(low_true, c.score)
                    else:
                        high_false = max(high_false, c.score)
        res[str(db)] = {"windows": total, "missed": miss, "lowest_true_score_that_won": low_true, "highest_false_score_that_won": high_false}
        print(json.dumps({str(db): res[str(db)]}), flush=True)
    return res


def model(a) -> dict:
    from meteor_demod_amd import interleave as il
    m = min(a.symbols[0], 1 << 22)
    soft = _stream(m)
    t0 = time.perf_counter()
    cand = il.model_candidates(soft)
    t1 = time.perf_counter()
    segs, P = il.track(cand, m)
    t2 = time.perf_counter()
    il.model_deinterleave(soft, segs, P)
    t3 = time.perf_counter()
    return {"symbols": m, "candidates_seconds": t1 - t0, "candidates_msymbols_per_s": m / (t1 - t0) / 1e6, "track_seconds": t2 - t1,
            "deinterleave_seconds": t3 - t2, "deinterleave_msymbols_per_s": m / (t3 - t2) / 1e6, "segments": len(segs), "periods": P}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["gpu", "threshold", "model", "all"])
    ap.add_argument("--symbols", type=_n, nargs="+", default=[1 << 26])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--out", type=Path, help="also write the JSON here")
    a = ap.parse_args()
    if a.what in ("gpu", "all"):
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: nothing here is timed on the CPU")
    steps = {"gpu": gpu, "threshold": threshold, "model": model}
    r = {k: f(a) for k, f in steps.items() if a.what in (k, "all")}
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
