"""Rates of the map layer (include/meteor_demod_amd_map.h); numbers go to profiles/map.md.

    python tools/map_rate.py host [--rows 600 --scale 100]
        the host's time for the time fit and the node grid of the mid-latitude pass of tests/map_util.py (no GPU).
    python tools/map_rate.py gpu [--rows 600 --scale 100 --reps 5]
        three random pictures of that many strip rows (600: a pass of 4800 lines, the input of profiles/picture.md) in device
        memory, nine cells in ten filled, on the grid of that pass.  mdemod_map_warp_device for 3 planes and for 1 plane, and
        mdemod_picture_render_device for 3 planes on the same inputs, each between two device events, `reps` calls after a
        warm-up, all of them reported; the warp's result (pixels and valid) is checked against the host model.  Bytes: what the kernel must move - the part of the selected slots that
        the grid looks at, the nodes, planes x W bytes a line out and the valid bytes - over the best time.  Run it under
        rocprofv3 --kernel-trace --stats (a run of its own) for the kernels' own times.
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

def the_grid(rows: int, scale: float):
    import map_util as MU
    from meteor_demod_amd import map as M
    place, info = MU.packets(rows, MU.mid_latitude_s0())
    M.make_opts()                                                                  # (the library is loaded before the clock starts)
    t0 = time.perf_counter()
    timing = M.fit_time(place, info)
    t1 = time.perf_counter()
    g = M.grid(MU.tle_text(), timing, 8 * rows, px_per_deg=scale)
    t2 = time.perf_counter()
    there = int(((g.nodes[..., 0] != M.NO_NODE) | (g.nodes[..., 1] != M.NO_NODE)).sum())
    return g, dict(rows=rows, scale=scale, width=g.width, height=g.height, sx=g.sx, nodes=list(g.nodes.shape[:2]), nodes_there=there, packets=int(place.size),
                   fit_ms=1e3 * (t1 - t0), grid_ms=1e3 * (t2 - t1))


def gpu(rows: int, scale: float, reps: int) -> dict:
    import torch
    from meteor_demod_amd import map as M, picture
    assert torch.cuda.is_available(), "map_rate.py gpu needs a GPU"
    g, out = the_grid(rows, scale)
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8) for _ in range(3)]
    filled = [(rng.random((rows, 14)) < 0.9).astype(np.uint8) for _ in range(3)]
    d_images, d_filled = [torch.from_numpy(x).cuda() for x in images], [torch.from_numpy(x).cuda() for x in filled]
    luts = np.stack([picture.lut(h) for h in picture.model_histogram(images, filled)])
    d_luts, d_nodes = torch.from_numpy(luts).cuda(), torch.from_numpy(g.nodes).cuda()
    cmap = picture.column_map()
    d_cmap = torch.from_numpy(cmap.view(np.int32)).cuda()
    w, h = g.width, g.height
    out["reps"] = reps

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return res, times

    t0 = time.perf_counter()
    want, want_val = M.model_warp(images, filled, (2, 1, 0), luts, g.nodes, w, h, valid=True)
    out["model_ms"] = 1e3 * (time.perf_counter() - t0)
    inside = int(np.count_nonzero(want_val))
    out["valid_share"] = inside / want_val.size
    (px, val), t = timed(lambda: M.warp(d_images, d_filled, (2, 1, 0), d_luts, d_nodes, w, h, valid=True))
    assert np.array_equal(px.cpu().numpy(), want) and np.array_equal(val.cpu().numpy(), want_val), "the colour warp differs from the model"
    # every source byte once, the nodes, the tables; every output byte
    moved = 3 * (8 * rows * 1568 + rows * 14) + g.nodes.size * 4 + 768 + h * w * 3 + h * w
    out["warp_3"] = dict(ms=t, best_ms=min(t), bytes=moved, gb_per_s=moved / min(t) / 1e6)
    (px, val), t = timed(lambda: M.warp(d_images, d_filled, (1,), d_luts[:1], d_nodes, w, h, valid=True))
    grey, grey_val = M.model_warp(images, filled, (1,), luts[:1], g.nodes, w, h, valid=True)
    assert np.array_equal(px.cpu().numpy(), grey) and np.array_equal(val.cpu().numpy(), grey_val), "the grey warp differs from the model"
    moved = 8 * rows * 1568 + rows * 14 + g.nodes.size * 4 + 256 + 2 * h * w
    out["warp_1"] = dict(ms=t, best_ms=min(t), bytes=moved, gb_per_s=moved / min(t) / 1e6)
    _, t = timed(lambda: picture.render(d_images, d_filled, (2, 1, 0), d_luts, d_cmap, valid=True))
    pw = int(cmap.size)
    moved = 3 * (8 * rows * 1568 + rows * 14) + 8 * rows * pw * 3 + rows * pw + 768 + 4 * pw
    out["picture_render_3"] = dict(width=pw, ms=t, best_ms=min(t), bytes=moved, gb_per_s=moved / min(t) / 1e6)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "gpu"])
    ap.add_argument("--rows", type=int, default=600)
    ap.add_argument("--scale", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(the_grid(a.rows, a.scale)[1] if a.what == "host" else gpu(a.rows, a.scale, a.reps)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
