"""Times of the equalise layer on the GPU, for profiles/equalise.md.

    python tools/equalise_rate.py [--width 8192 --height 4096] [--reps 7] [--batch 10] [--no-check]

One process, one device.  A synthetic picture (smooth ground, edges, noise of sigma 6; and a flat one, the worst case of the LDS
atomics) of three planes through mdemod_equalise_tables_device, mdemod_equalise_apply_device and both, at the defaults (tile 128,
luminance) and at tile 16 and tile 512, and at the defaults for mode "planes" and for one plane.  Every time is that of `batch` calls
between two device events after a warm-up, divided by `batch`; the best and the median of `reps` such windows are printed.  Beside
them, in the same run, the picture layer's render (mdemod_picture_render_device) of a picture of the same size.  The defaults are
checked against the host model byte for byte before they are timed.  Prints one JSON line per configuration.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def the_picture(w: int, h: int, planes: int) -> np.ndarray:
    rng = np.random.default_rng(w + h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 128 + 70 * np.sin(xx / 37.0) * np.cos(yy / 51.0) + 40 * np.sin((xx + 2 * yy) / 230.0) + 30 * ((xx // 130 + yy // 90) % 2)
    if planes == 1:
        return np.clip(base + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)
    return np.clip(np.stack([base, 0.8 * base + 30, 255 - base], axis=2) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch
    from meteor_demod_amd import equalise as E, picture as P
    assert torch.cuda.is_available(), "equalise_rate.py needs a GPU"
    w, h = args.width, args.height
    st = lambda: C.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.batch):
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / args.batch)
        return dict(best_ms=round(min(times), 4), median_ms=round(statistics.median(times), 4))

    pictures = {3: the_picture(w, h, 3), 1: the_picture(w, h, 1)}
    flat = np.full((h, w, 3), 77, np.uint8)
    configs = [("defaults", pictures[3], dict()), ("tile 16", pictures[3], dict(tile=16)), ("tile 512", pictures[3], dict(tile=512)),
               ("mode planes", pictures[3], dict(mode="planes")), ("one plane", pictures[1], dict()), ("flat picture", flat, dict())]
    for name, pic, kw in configs:
        opts = E.options(**kw)
        planes = 1 if pic.ndim == 2 else 3
        need = E.workspace(w, h, planes, opts)
        d_pic = torch.from_numpy(pic).cuda()
        d_out = torch.empty_like(d_pic)
        d_work = torch.empty(need, dtype=torch.uint8, device="cuda")
        p, o, wk = C.c_void_p(d_pic.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_work.data_ptr())
        lib = E.lib()
        tables = lambda: lib.mdemod_equalise_tables_device(p, None, w, h, planes, C.byref(opts), wk, need, 0, st())
        apply = lambda: lib.mdemod_equalise_apply_device(p, None, w, h, planes, C.byref(opts), wk, o, 0, st())
        both = lambda: lib.mdemod_equalise_device(p, None, w, h, planes, C.byref(opts), wk, need, o, 0, st())
        assert both() == 0
        out = dict(config=name, width=w, height=h, planes=planes, tile=opts.tile, mode=opts.mode, workspace=need, reps=args.reps, batch=args.batch)
        if name == "defaults" and not args.no_check:
            want_work = E.model_workspace(pic, None, opts)
            want = E.model_apply(pic, None, work=want_work, **kw)
            assert np.array_equal(d_work.cpu().numpy()[:need], want_work[:need]), "the workspace differs from the model"
            assert np.array_equal(d_out.cpu().numpy(), want), "the output differs from the model"
            out["checked_against_model"] = True
        out["tables"], out["apply"], out["both"] = timed(tables), timed(apply), timed(both)
        # the traffic floor: the picture read twice and written once
        out["floor_bytes"] = 3 * pic.size
        out["gb_per_s_at_best"] = round(3 * pic.size / out["both"]["best_ms"] / 1e6, 1)
        print(json.dumps(out), flush=True)
        del d_pic, d_out, d_work

    # the picture layer's render of a picture of the same size: three slots of h lines through a map of w columns
    rng = np.random.default_rng(1)
    rows = h // 8
    images = [torch.from_numpy(rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8)).cuda() for _ in range(3)]
    filled = [torch.from_numpy((rng.random((rows, 14)) < 0.9).astype(np.uint8)).cuda() for _ in range(3)]
    luts = torch.from_numpy(np.stack([np.arange(256, dtype=np.uint8)] * 3)).cuda()
    ww = w // 4 * 4
    cmap = torch.from_numpy(((np.arange(ww, dtype=np.int64) * 1567 * 256) // max(ww - 1, 1)).astype(np.int32)).cuda()
    out = dict(config="picture_render", width=ww, height=8 * rows, planes=3)
    out.update(timed(lambda: P.render(images, filled, (2, 1, 0), luts, cmap, valid=True)))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
