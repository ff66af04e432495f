"""Rates of the transfer-frame layer (include/meteor_demod_amd_rs.h); numbers go to profiles/rs.md.

    python tools/rs_rate.py gpu [--frames 8192 --reps 3] [--no-model]
        that many CADUs in device memory (64 different encoded frames, repeated) under three loads:
          clean           no byte error anywhere: every wave leaves after its syndromes
          errors8         8 byte errors in every codeword: every wave runs Berlekamp-Massey, Chien and Forney
          uncorrectable   40 byte errors in every codeword: every wave runs them and gives up
        mdemod_rs_decode_device between two device events (the kernel rs_decode and nothing else), `reps` calls after a warm-up;
        the reports are checked (all 0, all 8, all 255).  model: the host model (mdemod_rs_model_decode) on one core, 256 frames
        of each load.  The yardstick is mdemod_frames_viterbi_device on as many frames: tools/frames_rate.py gpu --symbols 2^26
        --no-demod --no-model in the same session.  Run it under rocprofv3 --kernel-trace --stats (a run of its own, --no-model)
        for the kernel's own times.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

LOADS = {"clean": 0, "errors8": 8, "uncorrectable": 40}


def _batch(n: int, errors: int) -> np.ndarray:
    """n CADUs: 64 encoded frames with `errors` byte errors in every codeword, the same 64 over and over."""
    import rs_util as R
    from meteor_demod_amd import rs
    rng = np.random.default_rng(7 + errors)
    base = np.stack([rs.model_encode(R.vcdu(rng, counter=k)) for k in range(64)])
    for row in base:
        for c in range(4):
            R.damage(row, c, errors, rng)
    return np.ascontiguousarray(np.tile(base, ((n + 63) // 64, 1))[:n])


def gpu(a) -> dict:
    import torch
    from meteor_demod_amd import rs
    from meteor_demod_amd._capi import check
    lib, st = rs.lib(), C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    n, out = a.frames, {"frames": a.frames}
    vcdu = torch.empty((n, 892), dtype=torch.uint8, device="cuda:0")
    info = torch.empty((n, 8), dtype=torch.uint8, device="cuda:0")
    for name, errors in LOADS.items():
        cadu = _batch(n, errors)
        d = torch.from_numpy(cadu).cuda()

        def call():
            check(lib.mdemod_rs_decode_device(None, C.c_void_p(d.data_ptr()), n, C.c_void_p(vcdu.data_ptr()), C.c_void_p(info.data_ptr()), 0, st), name)
        call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        got = info.cpu().numpy()
        want = errors if errors <= 16 else 255
        assert (got[:, :4] == want).all() and (got[:, 4] == (want == 255)).all(), (name, got[:2])
        r = {"errors_per_codeword": errors, "seconds": [round(t, 6) for t in ts], "best_seconds": min(ts), "frames_per_s": n / min(ts),
             "input_gb_per_s": n * 1024 / min(ts) / 1e9}
        if not a.no_model:
            k = min(n, 256)
            t0 = time.perf_counter()
            rs.model_decode(cadu[:k])
            t = time.perf_counter() - t0
            r["model_one_core"] = {"frames": k, "seconds": round(t, 6), "frames_per_s": k / t}
        out[name] = r
        print(json.dumps({name: r}), flush=True)
        del d
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["gpu"])
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", type=Path, help="also write the JSON here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured on the CPU")
    line = json.dumps({a.what: gpu(a)})
    print(line, flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
