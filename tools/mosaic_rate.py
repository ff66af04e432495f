"""Rates of the mosaic layer (include/meteor_demod_amd_mosaic.h); numbers go to profiles/mosaic.md.

    python tools/mosaic_rate.py host [--rows 600 --scale 100 --passes 3]
        the host's time for the time fits, the common grid and every pass's nodes of overlapping mid-latitude passes (the pass of
        tests/map_util.py, and the same orbit with its node 8 and 16 degrees further east, 20 and 40 row periods later).  No GPU.
    python tools/mosaic_rate.py gpu [--rows 600 --scale 100 --reps 5]
        for 2 and for 3 of those passes: three random pictures per pass of that many strip rows in device memory, nine cells in ten
        filled, on the common grid.  mdemod_mosaic_blend_device (3 planes, valid and cover; feather, then best; then 1 plane) against n launches of
        mdemod_map_warp_device through the same nodes onto the same grid (the per-pass maps a blend on the host would start from),
        alternating, each between two device events, `reps` times after a warm-up, all of them reported; the blend's result is
        checked against the host model.  Bytes: what the kernel must move - the part of the selected slots inside the grid counted
        as all of them, the nodes, the tables, every output byte once - over the best time.  Run it under rocprofv3 --kernel-trace
        --stats (a run of its own) for the kernels' own times.
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


def the_passes(rows: int, n: int, seed: int = 1):
    import map_util as MU
    from meteor_demod_amd import mosaic as M
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        place, info = MU.packets(rows, MU.mid_latitude_s0() + 20 * k * MU.ROW_PERIOD)
        images = [rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8) for _ in range(3)]
        filled = [(rng.random((rows, 14)) < 0.9).astype(np.uint8) for _ in range(3)]
        out.append(M.Pass(MU.with_raan(150.0 + 8.0 * k), images, filled, place, info))
    return out


def the_grid(passes, scale: float):
    from meteor_demod_amd import mosaic as M
    M.make_opts()                                                                  # (the library is loaded before the clock starts)
    t0 = time.perf_counter()
    g = M.grid(passes, px_per_deg=scale)
    t1 = time.perf_counter()
    there = [int(((n[..., 0] != M.NO_NODE) | (n[..., 1] != M.NO_NODE)).sum()) for n in g.nodes]
    return g, dict(passes=len(passes), scale=scale, width=g.width, height=g.height, sx=g.sx, nodes=list(g.nodes.shape[1:3]), nodes_there=there, grid_ms=1e3 * (t1 - t0))


def gpu(rows: int, scale: float, reps: int) -> dict:
    import torch
    from meteor_demod_amd import map as MP, mosaic as M, picture
    assert torch.cuda.is_available(), "mosaic_rate.py gpu needs a GPU"
    out = dict(rows=rows, reps=reps)
    select = (2, 1, 0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        return res, a.elapsed_time(b)

    for n in (2, 3):
        passes = the_passes(rows, n)
        g, rec = the_grid(passes, scale)
        w, h = g.width, g.height
        luts = [np.stack([picture.lut(x) for x in picture.model_histogram(p.images, p.filled)]) for p in passes]
        host = [(p.images, p.filled, luts[k], g.nodes[k]) for k, p in enumerate(passes)]
        dev = [([torch.from_numpy(x).cuda() for x in p.images], [torch.from_numpy(x).cuda() for x in p.filled], torch.from_numpy(luts[k]).cuda(),
                torch.from_numpy(g.nodes[k]).cuda()) for k, p in enumerate(passes)]
        t0 = time.perf_counter()
        want = M.model_blend(host, select, w, h, "feather", valid=True, cover=True)
        rec["model_ms"] = 1e3 * (time.perf_counter() - t0)
        rec["valid_share"] = float(np.count_nonzero(want[1])) / want[1].size
        rec["overlap_share"] = float(((want[2] & (want[2] - 1)) != 0).sum()) / want[2].size
        blend = lambda mode: M.blend(dev, select, w, h, mode, valid=True, cover=True)
        warps = lambda: [MP.warp(d[0], d[1], select, d[2], d[3], w, h, valid=True) for d in dev]
        got = blend("feather")
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got, want)), "the blend differs from the model"
        best_want = M.model_blend(host, select, w, h, "best", valid=True, cover=True)
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(blend("best"), best_want)), "the best-pass blend differs from the model"
        warps()
        torch.cuda.synchronize()
        times = dict(feather=[], best=[], warps=[])
        for _ in range(reps):                                                      # alternating: the three see the same machine
            times["feather"].append(timed(lambda: blend("feather"))[1])
            times["warps"].append(timed(warps)[1])
            times["best"].append(timed(lambda: blend("best"))[1])
        source = n * (3 * (8 * rows * 1568 + rows * 14) + g.nodes[0].size * 4 + 768)
        moved = dict(feather=source + h * w * 5, best=source + h * w * 5, warps=source + n * h * w * 4)
        for name, t in times.items():
            rec[name] = dict(ms=t, best_ms=min(t), bytes=moved[name], gb_per_s=moved[name] / min(t) / 1e6)
        rec["blend_over_warps"] = min(times["feather"]) / min(times["warps"])
        # grey: one plane of the same passes (the instance with the fewest registers)
        grey = dict(feather_1=[], warps_1=[])
        blend_1 = lambda: M.blend([(d[0], d[1], d[2][:1], d[3]) for d in dev], (1,), w, h, "feather", valid=True, cover=True)
        warps_1 = lambda: [MP.warp(d[0], d[1], (1,), d[2][:1], d[3], w, h, valid=True) for d in dev]
        blend_1(), warps_1()
        torch.cuda.synchronize()
        for _ in range(reps):
            grey["feather_1"].append(timed(blend_1)[1])
            grey["warps_1"].append(timed(warps_1)[1])
        for name, t in grey.items():
            rec[name] = dict(ms=t, best_ms=min(t))
        rec["blend_over_warps_1"] = min(grey["feather_1"]) / min(grey["warps_1"])
        out[f"passes_{n}"] = rec
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "gpu"])
    ap.add_argument("--rows", type=int, default=600)
    ap.add_argument("--scale", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(the_grid(the_passes(a.rows, a.passes), a.scale)[1] if a.what == "host" else gpu(a.rows, a.scale, a.reps)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
