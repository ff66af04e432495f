"""Measurements of the frame layer's link variant (include/meteor_demod_amd_frames_link.h); numbers go to profiles/frames_link.md.

    python tools/frames_link_rate.py gpu [--symbols 2^26 --reps 3] [--no-demod]
        one framed stream of that many soft symbols (128 frames at Es/N0 7 dB, repeated) in device memory, one process:
          candidates   mdemod_frames_candidates_device (the yardstick) and mdemod_frames_link_candidates_device with differential,
                       with skew (24 H) and with both (12 H), each between two device events
          viterbi      mdemod_frames_viterbi_device (the yardstick) and mdemod_frames_link_viterbi_device with skew and with both, on
                       the same frame list, host clock around the synchronous call
          demodulate   mdemod_demodulate_recording of a recording of as many symbols (OQPSK 72 ksym/s at 288 kS/s, s16, 12 dB), host
                       clock: the step the frame layer follows
    python tools/frames_link_rate.py threshold [--seeds 3]
        the share of windows whose argmax is not the true marker, per Es/N0: 8-way (plain), 12-way (differential + skew) and 24-way
        (skew), on the GPU's candidates (they are the model's)
    python tools/frames_link_rate.py locks
        the NRZ-M OQPSK recording of tests/link_util.py at its four starting carrier phases through the GPU OQPSK demodulator and
        decode(skew, differential): which (h, s) the demodulator produced
    python tools/frames_link_rate.py all      the three in one run
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from frames_rate import SPS, _event_timed, _fig, _host_timed, _n, _stream  # noqa: E402

MODES = {"plain": (False, False), "differential": (True, False), "skew": (False, True), "differential+skew": (True, True)}


def gpu(a) -> dict:
    import torch
    from meteor_demod_amd import DemodConfig, frames, synth
    from meteor_demod_amd._capi import check
    from meteor_demod_amd.recording import demodulate_recording_native
    out = {}
    for m in a.symbols:
        soft = _stream(m)
        d = torch.from_numpy(soft).cuda()
        r = {"symbols": m}
        for name, (diff, skew) in MODES.items():
            r[f"candidates_{name}"] = _fig(_event_timed(lambda: frames.candidates_tensor(d, differential=diff, skew=skew), a.reps), m)
        found = frames.track(frames.candidates(d), m)
        r["frames"] = len(found)
        lib, st = frames.lib(), C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        arr = frames._to_c(found)
        cadu_dev = torch.empty((max(1, len(found)), 1024), dtype=torch.uint8, device=d.device)
        r["viterbi_plain"] = _fig(_host_timed(lambda: check(lib.mdemod_frames_viterbi_device(C.c_void_p(d.data_ptr()), m, arr, len(found),
                                                                                           C.c_void_p(cadu_dev.data_ptr()), 0, st), "viterbi"), a.reps), m)
        for name in ("skew", "differential+skew"):
            link = frames.make_link(*MODES[name])
            r[f"viterbi_{name}"] = _fig(_host_timed(lambda: check(lib.mdemod_frames_link_viterbi_device(
                C.byref(link), C.c_void_p(d.data_ptr()), m, arr, len(found), C.c_void_p(cadu_dev.data_ptr()), 0, st), "link viterbi"), a.reps), m)
        plain = r["candidates_plain"]["best_seconds"] + r["viterbi_plain"]["best_seconds"]
        for name in ("skew", "differential+skew"):
            both = r[f"candidates_{name}"]["best_seconds"] + r[f"viterbi_{name}"]["best_seconds"]
            r[f"{name}_over_plain"] = {"candidates": r[f"candidates_{name}"]["best_seconds"] / r["candidates_plain"]["best_seconds"],
                                       "viterbi": r[f"viterbi_{name}"]["best_seconds"] / r["viterbi_plain"]["best_seconds"], "both": both / plain}
        del d
        if not a.no_demod:
            cfg = DemodConfig(samplerate=72000 * SPS, oqpsk=True)
            sst = synth.make_stream(7, 72000 * SPS, 72000, f0_hz=300.0, esn0_db=12.0, rms=3000.0, dc=(0.0, 0.0))
            iq = synth.generate_device([sst], m * SPS)[0]
            torch.cuda.synchronize()
            syms = []

            def once():
                s, _ = demodulate_recording_native(cfg, iq)
                syms.append(int(s.shape[0]))
            r["demodulate_recording_call"] = {"samples": m * SPS, **_fig(_host_timed(once, min(a.reps, 2)), m), "symbols_out": syms[-1]}
            del iq
            for name in ("plain", "skew", "differential+skew"):
                t = r[f"candidates_{name}"]["best_seconds"] + r[f"viterbi_{name}"]["best_seconds"]
                r[f"{name}_over_demodulation"] = t / r["demodulate_recording_call"]["best_seconds"]
        torch.cuda.empty_cache()
        out[str(m)] = r
        print(json.dumps({str(m): r}), flush=True)
    return out


def threshold(a) -> dict:
    import torch
    import link_util as L
    from meteor_demod_amd import frames
    res = {}
    ways = {"8-way": (False, False, (0, 3, 5)), "24-way": (False, True, (0, 11, 21)), "12-way": (True, True, (0, 9, 20))}
    for db in (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0):
        res[str(db)] = {}
        for way, (diff, skew, hyps) in ways.items():
            miss = total = 0
            low_true, high_false = 1 << 30, 0
            for seed in range(a.seeds):
                st = L.LinkStream(seed=50 + seed, n_frames=32, lead=777, tail=300, differential=diff)
                for H in hyps:
                    soft = st.received(H, db, seed=1000 * seed + H)
                    c = frames.candidates(torch.from_numpy(soft).cuda(), differential=diff, skew=skew)[:32]
                    for k, x in enumerate(c):
                        ok = x.position == st.positions[k] and x.hypothesis == L.canonical(H, diff)
                        miss += not ok
                        total += 1
                        if ok:
                            low_true = min(low_true, x.score)
                        else:
                            high_false = max(high_false, x.score)
            res[str(db)][way] = {"windows": total, "missed": miss, "lowest_true_score_that_won": low_true, "highest_false_score_that_won": high_false}
        print(json.dumps({str(db): res[str(db)]}), flush=True)
    return res


def locks(a) -> dict:
    import torch
    import link_util as L
    from meteor_demod_amd import Demodulator, frames
    res = {}
    for phase in L.REC_PHASES:
        st, iq = L.recording(phase)
        with Demodulator(L.recording_cfg(), 1, 0) as dm:
            soft = dm.process_host([iq])[0]
        cadu, fr = frames.decode(torch.from_numpy(np.ascontiguousarray(soft)).cuda(), skew=True, differential=True)
        res[str(phase)] = {"symbols": int(len(soft)), "frames": len(fr), "as_sent": sum(bytes(c) in st.frames for c in cadu),
                           "h_s": sorted({(f.hypothesis & 7, f.hypothesis >> 3) for f in fr}),
                           "mean_channel_errors": float(np.mean([f.channel_errors for f in fr])) if fr else 0.0}
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["gpu", "threshold", "locks", "all"])
    ap.add_argument("--symbols", type=_n, nargs="+", default=[1 << 26])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--no-demod", action="store_true")
    ap.add_argument("--out", type=Path, help="also write the JSON here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured on the CPU")
    steps = {"gpu": gpu, "threshold": threshold, "locks": locks}
    r = {k: f(a) for k, f in steps.items() if a.what in (k, "all")}
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
