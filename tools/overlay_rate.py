"""Rates of the overlay layer (include/meteor_demod_amd_overlay.h); numbers go to profiles/overlay.md.

    python tools/overlay_rate.py host [--width 8192 --height 4096 --pieces 100000]
        the host's time to project, cut and bin a 5 degree graticule and a synthetic coast of about that many pieces for a picture
        of that size at 100 pixels per degree, and the histogram of items per tile (no GPU).
    python tools/overlay_rate.py gpu [--width 8192 --height 4096 --pieces 100000 --reps 5]
        the same, then mdemod_overlay_draw_device on a colour picture of that size in device memory and, beside it in the same
        process, mdemod_map_warp_device making a picture of that size from three random pictures of 600 strip rows through an
        affine node grid; each between two device events, `reps` calls after a warm-up, all of them reported.  The draw's bytes are
        checked against the host model through the tiles.  Bytes: what the draw must move - the pixels of the tiles with items in
        and out, the mask, the records and items of every tile - over the best time.
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


def the_lines(width: int, height: int, pieces: int):
    """The grid, the layers, the styles and the host's times.  The coast: random walks of 8 pixel steps (a vertex every 8 pixels is
    what a 1 : 10 million coastline has at 100 pixels per degree), 2000 vertices each, as many as make about `pieces` pieces."""
    from meteor_demod_amd import overlay as O
    g = O.Geo(width, height, 100, 100.0, 50.0, -20.0)
    rng = np.random.default_rng(4)
    walks = max(1, pieces // 2000)
    lines = []
    for _ in range(walks):
        n = 2000
        turn = np.cumsum(rng.normal(0, 0.25, n))
        x = rng.uniform(0, width) + np.cumsum(8 * np.cos(turn))
        y = rng.uniform(0, height) + np.cumsum(8 * np.sin(turn))
        lines.append((g.lon_left + x / g.sx, np.clip(g.lat_top - y / g.sy, -90, 90)))
    coast = O.vectors(lines)
    styles = O.default_styles()
    O.lib()                                                                        # (the library is loaded before the clock starts)
    t0 = time.perf_counter()
    grat = O.graticule(g, 5)
    layers = [(coast, 0), (grat, 1)]
    t1 = time.perf_counter()
    points = [O.project(g, v) for v, _ in layers]
    t2 = time.perf_counter()
    pcs = np.concatenate([O.pieces(p, s, styles[s].half_width, width, height) for p, (_, s) in zip(points, layers)])
    t3 = time.perf_counter()
    tile_first, items = O.bins(pcs, styles, width, height)
    t4 = time.perf_counter()
    per_tile = np.diff(tile_first.astype(np.int64))
    edges = [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 1 << 30]
    hist = {f"{a}..{b - 1}" if b < (1 << 30) else f"{a}..": int(((per_tile >= a) & (per_tile < b)).sum()) for a, b in zip(edges[:-1], edges[1:])}
    out = dict(width=width, height=height, vertices=int(coast.lon.size), pieces=int(pcs.size), pieces_per_style=[int((pcs["style"] == s).sum()) for s in range(2)],
               items=int(items.size), tiles=int(per_tile.size), tiles_with_items=int((per_tile > 0).sum()), most_in_a_tile=int(per_tile.max()), items_per_tile=hist,
               graticule_ms=1e3 * (t1 - t0), project_ms=1e3 * (t2 - t1), cut_ms=1e3 * (t3 - t2), bin_ms=1e3 * (t4 - t3))
    return g, styles, pcs, tile_first, items, out


def gpu(width: int, height: int, pieces: int, reps: int) -> dict:
    import torch
    import map_util as MU
    from meteor_demod_amd import map as M, overlay as O
    assert torch.cuda.is_available(), "overlay_rate.py gpu needs a GPU"
    g, styles, pcs, tile_first, items, out = the_lines(width, height, pieces)
    out["reps"] = reps
    rng = np.random.default_rng(1)
    pixels = rng.integers(0, 256, (height, width, 3), dtype=np.uint8)

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

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_pcs, d_first, d_items = up(pcs), up(tile_first), up(items)
    d_pixels = torch.from_numpy(pixels).cuda()
    t0 = time.perf_counter()
    want, want_mask = O.model_tiles(pixels, pcs, tile_first, items, styles)
    out["model_ms"] = 1e3 * (time.perf_counter() - t0)
    first = d_pixels.clone()
    mask = O.draw_pieces(first, d_pcs, d_first, d_items, styles, mask=True)
    assert np.array_equal(first.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy(), want_mask), "the draw differs from the model"
    out["pixels_drawn"] = [int(((want_mask >> s) & 1).sum()) for s in range(2)]
    # (in place: every call after the first draws on a drawn picture; the work is the same)
    _, t = timed(lambda: O.draw_pieces(first, d_pcs, d_first, d_items, styles, mask=True))
    busy = out["tiles_with_items"]
    moved = busy * 32 * 32 * 3 * 2 + height * width * 2 + out["items"] * (32 + 4) + tile_first.size * 4
    out["draw_3"] = dict(ms=t, best_ms=min(t), bytes=moved, gb_per_s=moved / min(t) / 1e6)
    _, t = timed(lambda: O.draw_pieces(first, d_pcs, d_first, d_items, styles))
    out["draw_3_no_mask"] = dict(ms=t, best_ms=min(t))
    # the warp of a picture of the same size: 600 strip rows spread over it
    rows = 600
    images = [rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8) for _ in range(3)]
    filled = [(rng.random((rows, 14)) < 0.9).astype(np.uint8) for _ in range(3)]
    d_images, d_filled = [torch.from_numpy(x).cuda() for x in images], [torch.from_numpy(x).cuda() for x in filled]
    luts = np.stack([np.arange(256, dtype=np.uint8)] * 3)
    fx, fy = (1567 * 256) // width, ((8 * rows - 1) * 256) // height
    nodes = MU.affine_nodes(width, height, lambda i, j: np.minimum(fx * j, 1567 * 256), lambda i, j: np.minimum(fy * i, (8 * rows - 1) * 256))
    d_luts, d_nodes = torch.from_numpy(luts).cuda(), torch.from_numpy(nodes).cuda()
    (px, val), t = timed(lambda: M.warp(d_images, d_filled, (2, 1, 0), d_luts, d_nodes, width, height, valid=True))
    out["warp_valid_share"] = float((val != 0).float().mean().item())
    moved = 3 * (8 * rows * 1568 + rows * 14) + nodes.size * 4 + 768 + height * width * 4
    out["warp_3"] = dict(ms=t, best_ms=min(t), bytes=moved, gb_per_s=moved / min(t) / 1e6)
    out["draw_over_warp"] = out["draw_3"]["best_ms"] / out["warp_3"]["best_ms"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "gpu"])
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--pieces", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(the_lines(a.width, a.height, a.pieces)[5] if a.what == "host" else gpu(a.width, a.height, a.pieces, a.reps)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
