"""Times of the sun layer on the GPU, for profiles/sun.md.

    python tools/sun_rate.py [--rows 731] [--reps 9] [--batch 50] [--no-check]

One process, one device.  A pass of `rows` strip rows (731: 15 minutes) of the golden element set, three slots of random bytes: the
gain nodes of the pass (host), then mdemod_sun_apply_device under slot mask 7 in place, beside it in the same run a device-to-device
copy of the same bytes (three slots), and the map layer's warp of that pass (mdemod_map_warp_device: three planes with the valid
mask, at 50 pixels per degree).  Every time is that of `batch` calls between two device events after a warm-up, divided by `batch`;
the three are taken in turn, `reps` windows each, and the best and the median are printed.  The apply is checked against the host
model, bytes and counts, before it is timed.  Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROW_PERIOD, TIME_OFFSET = 1.230769, 10800.0


def packets(rows: int, s0: float):
    """One placed packet per strip row, stamped s0 + row x period: what the time fit needs."""
    from meteor_demod_amd import map as M
    total = np.rint((s0 + ROW_PERIOD * np.arange(rows)) * 1e6).astype(np.int64) % (86400 * 10 ** 6)
    place = np.zeros(rows, dtype=M.PLACEMENT)
    info = np.zeros(rows, dtype=M.STRIP_INFO)
    place["row"] = np.arange(rows)
    info["ms"], info["us"] = total // 1000, total % 1000
    return place, info


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=731)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch
    from meteor_demod_amd import map as M, sun as S
    assert torch.cuda.is_available(), "sun_rate.py needs a GPU"
    rows = args.rows
    tle = M.parse_tle((ROOT / "tests" / "golden" / "map_tle.txt").read_text())
    # the ascending node is at the epoch: 150 degrees of argument of latitude later the golden orbit runs south over the day side
    period = 86400.0 / tle.mean_motion
    s0 = tle.epoch_sec + 150.0 / 360.0 * period + TIME_OFFSET
    opts = dict(date=tle.epoch_day, time_offset=TIME_OFFSET, px_per_deg=50)
    place, info = packets(rows, s0)
    timing = M.fit_time(place, info, **opts)
    t0 = time.perf_counter()
    gain, summ = S.nodes(tle, timing, rows, **opts)
    nodes_ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(what="nodes (host)", rows=rows, ms=round(nodes_ms, 2), **summ)), flush=True)

    rng = np.random.default_rng(rows)
    pics = [rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8) for _ in range(3)]
    d_in = torch.from_numpy(np.stack(pics)).cuda()
    d_out = torch.empty_like(d_in)
    d_gain = torch.from_numpy(gain.view(np.int32)).cuda()
    d_work = torch.zeros((rows, 3), dtype=torch.int32, device="cuda")
    need = S.workspace(rows)
    lib = S.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    slots = lambda t: (C.c_void_p * 3)(*[t[k].data_ptr() for k in range(3)])
    pi, po = slots(d_in), slots(d_out)
    apply = lambda: lib.mdemod_sun_apply_device(C.byref(pi), C.byref(po), 7, rows, C.c_void_p(d_gain.data_ptr()), C.c_void_p(d_work.data_ptr()), need, 0, st())
    assert apply() == 0
    if not args.no_check:
        want, wsat = S.model_apply(pics, gain, 7)
        got = d_out.cpu().numpy()
        assert all(np.array_equal(got[k], want[k]) for k in range(3)), "the output differs from the model"
        assert [int(v) for v in d_work.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=0)] == wsat, "the counts differ from the model"
    copy = lambda: d_out.copy_(d_in)

    grid = M.grid(tle, timing, 8 * rows, **opts)
    filled = [torch.ones((rows, 14), dtype=torch.uint8, device="cuda") for _ in range(3)]
    luts = torch.from_numpy(np.stack([np.arange(256, dtype=np.uint8)] * 3)).cuda()
    d_nodes = torch.from_numpy(grid.nodes).cuda()
    images = [d_in[k] for k in range(3)]
    warp = lambda: M.warp(images, filled, (2, 1, 0), luts, d_nodes, grid.width, grid.height, valid=True)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.batch

    todo = {"apply, 3 slots": apply, "device-to-device copy, 3 slots": copy, "map warp, 3 planes + valid": warp}
    times = {k: [] for k in todo}
    for fn in todo.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in todo.items():                                              # in turn: what else the machine does meets all three alike
            times[name].append(window(fn))
    nbytes = d_in.numel()
    best = {}
    for name, t in times.items():
        best[name] = min(t)
        out = dict(what=name, rows=rows, best_ms=round(min(t), 4), median_ms=round(statistics.median(t), 4), reps=args.reps, batch=args.batch)
        if name.startswith("map warp"):
            out.update(width=grid.width, height=grid.height, px_per_deg=50)
        else:
            out.update(bytes_read=nbytes, bytes_written=nbytes, gb_per_s_at_best=round(2 * nbytes / min(t) / 1e6, 1))
        print(json.dumps(out), flush=True)
    print(json.dumps(dict(what="ratios at best", apply_over_copy=round(best["apply, 3 slots"] / best["device-to-device copy, 3 slots"], 2),
                          apply_over_warp=round(best["apply, 3 slots"] / best["map warp, 3 planes + valid"], 3), checked_against_model=not args.no_check)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
