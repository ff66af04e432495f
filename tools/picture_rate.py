"""Rates of the picture layer (include/meteor_demod_amd_picture.h); numbers go to profiles/picture.md.

    python tools/picture_rate.py gpu [--rows 600 --reps 5]
        three random pictures of that many strip rows (600: a pass of 4800 lines) in device memory, nine cells in ten filled, the
        default map.  mdemod_picture_histogram_device (the memset and one kernel) and mdemod_picture_render_device (one kernel) for
        3 planes and for 1, each between two device events, `reps` calls after a warm-up, all of them reported; the histogram and
        the first and last 4 strip rows of each render are checked against the host model.  Bytes: what the kernel must move - the
        selected slots in, planes x W bytes a line out (and the valid bytes) - over the best time.  Run it under
        rocprofv3 --kernel-trace --stats (a run of its own) for the kernels' own times.
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


def gpu(rows: int, reps: int) -> dict:
    import torch
    from meteor_demod_amd import picture
    assert torch.cuda.is_available(), "picture_rate.py gpu needs a GPU"
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8) for _ in range(3)]
    filled = [(rng.random((rows, 14)) < 0.9).astype(np.uint8) for _ in range(3)]
    d_images, d_filled = [torch.from_numpy(x).cuda() for x in images], [torch.from_numpy(x).cuda() for x in filled]
    cmap = picture.column_map()
    w = int(cmap.size)
    hist_want = picture.model_histogram(images, filled)
    luts = np.stack([picture.lut(hist_want[s]) for s in range(3)])
    d_cmap, d_luts = torch.from_numpy(cmap.view(np.int32)).cuda(), torch.from_numpy(luts).cuda()
    out = dict(rows=rows, lines=8 * rows, width=w, reps=reps)

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

    hist, t = timed(lambda: picture.histogram(d_images, d_filled))
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), hist_want), "the histogram differs from the model"
    moved = 3 * 8 * rows * 1568 + 3 * rows * 14
    out["histogram"] = dict(ms=t, best_ms=min(t), bytes=moved, gb_per_s=moved / min(t) / 1e6)
    for select in ((2, 1, 0), (1,)):
        planes = len(select)
        (px, val), t = timed(lambda: picture.render(d_images, d_filled, select, d_luts[:planes], d_cmap, valid=True))
        px, val = px.cpu().numpy(), val.cpu().numpy()
        for at in (0, rows - 4):
            want, want_val = picture.model_render([x[8 * at: 8 * at + 32] for x in images], [x[at: at + 4] for x in filled], select, luts[:planes], cmap, valid=True)
            assert np.array_equal(px[8 * at: 8 * at + 32], want) and np.array_equal(val[at: at + 4], want_val), f"the render of {planes} planes differs from the model"
        moved = planes * (8 * rows * 1568 + rows * 14) + 8 * rows * w * planes + rows * w + 256 * planes + 4 * w
        out[f"render_{planes}"] = dict(ms=t, best_ms=min(t), bytes=moved, gb_per_s=moved / min(t) / 1e6,
                                       bytes_three_planes_in=3 * 8 * rows * 1568 + 8 * rows * w * planes)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gpu"])
    ap.add_argument("--rows", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(gpu(a.rows, a.reps)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
