"""Rates of the image layer (include/meteor_demod_amd_image.h); numbers go to profiles/image.md.

    python tools/image_rate.py gpu [--frames 8192 --reps 3] [--no-model] [--step-timeout 300]
        that many VCDUs in device memory (the frames of a 2^26-symbol stream), full of image packets, under three loads:
          clean       smooth, flat, noisy and edged strips at q = 80
          truncated   the same packets, every one cut in the middle (its length field says so): every lane stops half way
          noisy100    noise strips at q = 100: the longest bit streams, about 1400 bytes a packet
        mdemod_packets_find_device and mdemod_image_decode_device each between two device events, `reps` calls after a warm-up,
        all of them reported; the descriptors are checked against the host model on the whole batch, strips and reports on a
        sample of 512 packets.  model: the host model on one core, 1024 packets of each load.  Every load runs in a child process
        of its own under --step-timeout seconds, and the first that fails ends the run.  The yardstick is
        mdemod_frames_viterbi_device on as many frames: tools/frames_rate.py gpu --symbols 2^26 --no-demod --no-model in the same
        session.  Run one load under rocprofv3 --kernel-trace --stats (a run of its own: `one --load clean --no-model`) for the
        kernels' own times.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

LOADS = ("clean", "truncated", "noisy100")
ZONE = 882


def _batch(n: int, load: str):
    """(vcdu [n, 892], packets in them): 256 different packets over and over, sequence counts running, idle fill at the end."""
    import image_util as I
    from meteor_demod_amd import image
    base = []
    for i in range(256):
        kind, q = ("noise", 100) if load == "noisy100" else (I.KINDS[i % 4], 80)
        p = image.model_encode_packet(I.strip(kind, i), q, 14 * (i % 14), 64 + i % 3, 0, 1, i, 0)
        if load == "truncated":
            k = 20 + (len(p) - 20) // 2
            p = p[:4] + bytes([(k - 7) >> 8, (k - 7) & 0xFF]) + p[6:k]
        base.append(bytearray(p))
    parts, size, seq = [], 0, 0
    while size < n * ZONE - 70000:
        p = base[seq % 256]
        p[2], p[3] = 0xC0 | (seq >> 8) & 0x3F, seq & 0xFF
        parts.append(bytes(p))
        size += len(p)
        seq += 1
    while size < n * ZONE:
        room = min(n * ZONE - size, 60000)
        if 0 < n * ZONE - size - room < 7:
            room -= 7
        parts.append(I.idle_packet(room))
        size += room
    stream = np.frombuffer(b"".join(parts), dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]])
    first = np.searchsorted(starts, np.arange(n) * ZONE)                                  # the first header at or behind each frame's start
    fhp = np.where((first < len(starts)) & (starts[np.minimum(first, len(starts) - 1)] < (np.arange(n) + 1) * ZONE),
                   starts[np.minimum(first, len(starts) - 1)] - np.arange(n) * ZONE, 0x7FF)
    vcdu = np.zeros((n, 892), dtype=np.uint8)
    c = np.arange(n)
    vcdu[:, 0], vcdu[:, 1] = 0x40 | (0x9D >> 2), ((0x9D & 3) << 6) | 5
    vcdu[:, 2], vcdu[:, 3], vcdu[:, 4] = c >> 16, (c >> 8) & 0xFF, c & 0xFF
    vcdu[:, 8], vcdu[:, 9] = fhp >> 8, fhp & 0xFF
    vcdu[:, 10:] = stream.reshape(n, ZONE)
    return vcdu, len(parts)


def one(a) -> dict:
    import torch
    from meteor_demod_amd import image
    from meteor_demod_amd._capi import check
    lib, st = image.lib(), C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    n = a.frames
    vcdu, sent = _batch(n, a.load)
    want = image.model_find(vcdu)
    assert len(want) == sent, (len(want), sent)
    m = len(want)
    d_v = torch.from_numpy(vcdu).cuda()
    d_desc = torch.zeros((m, 16), dtype=torch.uint8, device="cuda:0")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_strips = torch.empty((m, 896), dtype=torch.uint8, device="cuda:0")
    d_sinfo = torch.empty((m, 16), dtype=torch.uint8, device="cuda:0")

    def find():
        check(lib.mdemod_packets_find_device(None, C.c_void_p(d_v.data_ptr()), None, n, C.c_void_p(d_desc.data_ptr()), m, C.c_void_p(d_total.data_ptr()), 0, st), "find")

    def decode():
        check(lib.mdemod_image_decode_device(None, C.c_void_p(d_v.data_ptr()), n, C.c_void_p(d_desc.data_ptr()), m, C.c_void_p(d_strips.data_ptr()),
                                             C.c_void_p(d_sinfo.data_ptr()), 0, st), "decode")

    def timed(call):
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
        return ts

    t_find, t_decode = timed(find), timed(decode)
    assert int(d_total.item()) == m and np.array_equal(image.descriptors(d_desc), want)
    pick = np.linspace(0, m - 1, min(m, 512)).astype(int)
    want_s, want_i = image.model_decode(vcdu, want[pick])
    got_i = image.strip_infos(d_sinfo)
    assert np.array_equal(d_strips.cpu().numpy()[pick].reshape(-1, 8, 112), want_s) and np.array_equal(got_i[pick], want_i)
    r = {"load": a.load, "frames": n, "packets": m, "mean_packet_bytes": round(float(want["length"].mean()), 1), "blocks_decoded": int(got_i["mcus"].sum()),
         "bits_used": int(got_i["bits_used"].astype(np.int64).sum()),
         "find_seconds": [round(t, 6) for t in t_find], "decode_seconds": [round(t, 6) for t in t_decode],
         "find_frames_per_s": n / min(t_find), "decode_packets_per_s": m / min(t_decode)}
    if not a.no_model:
        k = min(m, 1024)
        t0 = time.perf_counter()
        image.model_find(vcdu)
        t1 = time.perf_counter()
        image.model_decode(vcdu, want[:k])
        t2 = time.perf_counter()
        r["model_one_core"] = {"find_seconds": round(t1 - t0, 6), "find_frames_per_s": n / (t1 - t0), "decode_packets": k, "decode_seconds": round(t2 - t1, 6),
                               "decode_packets_per_s": k / (t2 - t1)}
    return r


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["gpu", "one"])
    ap.add_argument("--load", choices=LOADS, default="clean")
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", type=Path, help="also write the JSON here")
    a = ap.parse_args()
    if a.what == "one":
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: nothing here is measured on the CPU")
        print(json.dumps(one(a)), flush=True)
        return
    out = {}
    for load in LOADS:
        cmd = [sys.executable, str(Path(__file__).resolve()), "one", "--load", load, "--frames", str(a.frames), "--reps", str(a.reps)] + (["--no-model"] if a.no_model else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{load}: exit status {p.returncode}; nothing more is started")
        out[load] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps({load: out[load]}), flush=True)
    line = json.dumps({"gpu": out})
    print(line, flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
