"""Rates of the JPEG encoder (include/meteor_demod_amd_jpeg.h); numbers go to profiles/jpeg.md.

    python tools/jpeg_rate.py gpu [--reps 5] [--sizes 1568x1440x1,2784x1440x3,8192x4096x3] [--quality 90]
        per size, inside one process: mdemod_jpeg_encode_device on a synthetic picture in device memory (smooth ground, edges, noise
        of sigma 6) between two device events, `reps` calls after a warm-up; the entropy stage alone on the same coefficients
        (mdemod_jpeg_entropy_device: length pass, offsets, write pass) and once more with out_room 0, where the write pass returns at
        once (length pass and offsets); the transform is the difference.  Beside them mdemod_map_warp_device making a picture of the
        same size (the yardstick of profiles/overlay.md), libjpeg through PIL on one CPU core where PIL imports, and the host path:
        mdemod_jpeg_encode_host plus writing the .jpg against writing the same pixels as a binary P5 / P6 file.  The file is checked
        against the host model byte for byte.
    python tools/jpeg_rate.py gpu --only-encode --no-check --sizes 8192x4096x3
        the calls of mdemod_jpeg_encode_device alone: what a kernel trace of the four kernels is taken on, one size a process.
"""
from __future__ import annotations

import argparse
import io
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def the_picture(w: int, h: int, planes: int) -> np.ndarray:
    rng = np.random.default_rng(w + h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 128 + 70 * np.sin(xx / 37.0) * np.cos(yy / 51.0) + 40 * np.sin((xx + 2 * yy) / 230.0) + 30 * ((xx // 130 + yy // 90) % 2)
    if planes == 1:
        return np.clip(base + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)
    return np.clip(np.stack([base, 0.8 * base + 30, 255 - base], axis=2) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def gpu(sizes, quality: int, reps: int, check: bool, only_encode: bool = False) -> list:
    import ctypes as C
    import torch
    import map_util as MU
    from meteor_demod_amd import jpeg as J, map as M
    assert torch.cuda.is_available(), "jpeg_rate.py gpu needs a GPU"
    st = lambda: C.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return times

    results = []
    for w, h, planes in sizes:
        pic = the_picture(w, h, planes)
        d_pic = torch.from_numpy(pic).cuda()
        out = dict(width=w, height=h, planes=planes, quality=quality, reps=reps)
        t0 = time.perf_counter()
        got = J.encode_tensor(d_pic, quality)
        out["first_call_ms"] = 1e3 * (time.perf_counter() - t0)
        out["file_bytes"] = len(got)
        if check:
            t0 = time.perf_counter()
            want = J.model_encode(pic, quality)
            out["model_ms"] = 1e3 * (time.perf_counter() - t0)
            assert got == want, "the file differs from the model"
        n_mcus = ((w + 7) // 8) * ((h + 7) // 8)
        room, need = len(got) + 64, J.workspace(w, h, planes)
        d_out = torch.empty(room, dtype=torch.uint8, device="cuda")
        d_work = torch.empty(need, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(2, dtype=torch.int64, device="cuda")
        enc = lambda: J.lib().mdemod_jpeg_encode_device(C.c_void_p(d_pic.data_ptr()), w, h, planes, quality, 0, C.c_void_p(d_out.data_ptr()), room, C.c_void_p(d_res.data_ptr()),
                                                        C.c_void_p(d_work.data_ptr()), need, 0, st())
        t_all = timed(enc)
        assert d_out[: len(got)].cpu().numpy().tobytes() == got
        if only_encode:
            out["ms"] = dict(all=t_all)
            results.append(out)
            print(json.dumps(out), flush=True)
            continue
        # the coefficients lie at the head of the workspace: the entropy stage alone, with a workspace of its own
        coef_bytes = n_mcus * planes * 128
        d_coef = d_work[:coef_bytes].clone()
        need2 = int(J.lib().mdemod_jpeg_entropy_workspace(n_mcus, 0))
        d_work2 = torch.empty(need2, dtype=torch.uint8, device="cuda")
        ent = lambda r: J.lib().mdemod_jpeg_entropy_device(C.c_void_p(d_coef.data_ptr()), n_mcus, planes, 0, C.c_void_p(d_out.data_ptr()), r, C.c_void_p(d_res.data_ptr()),
                                                           C.c_void_p(d_work2.data_ptr()), need2, 0, st())
        t_ent, t_len = timed(lambda: ent(room)), timed(lambda: ent(0))
        segs = -(-n_mcus // 32)
        best = dict(all=min(t_all), entropy=min(t_ent), lengths_and_offsets=min(t_len))
        best["transform"] = best["all"] - best["entropy"]
        best["write"] = best["entropy"] - best["lengths_and_offsets"]
        out["ms"] = dict(all=t_all, entropy=t_ent, lengths_and_offsets=t_len)
        out["best_ms"] = best
        moved = dict(transform=pic.size + coef_bytes, lengths_and_offsets=coef_bytes + segs * 4 + segs * 12, write=coef_bytes + segs * 8 + len(got))
        out["bytes"] = moved
        out["gb_per_s"] = {k: moved[k] / best[k] / 1e6 for k in moved if best[k] > 0}
        out["entropy_share"] = best["entropy"] / best["all"]
        # the warp of a picture of the same size (tools/overlay_rate.py)
        rng = np.random.default_rng(1)
        rows = 600
        images = [torch.from_numpy(rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8)).cuda() for _ in range(3)]
        filled = [torch.from_numpy((rng.random((rows, 14)) < 0.9).astype(np.uint8)).cuda() for _ in range(3)]
        luts = torch.from_numpy(np.stack([np.arange(256, dtype=np.uint8)] * 3)).cuda()
        ww = (w + 3) // 4 * 4
        fx, fy = (1567 * 256) // ww, ((8 * rows - 1) * 256) // h
        nodes = torch.from_numpy(MU.affine_nodes(ww, h, lambda i, j: np.minimum(fx * j, 1567 * 256), lambda i, j: np.minimum(fy * i, (8 * rows - 1) * 256))).cuda()
        # (always the colour warp: three planes of that size, also beside a grey picture)
        t_warp = timed(lambda: M.warp(images, filled, (2, 1, 0), luts, nodes, ww, h, valid=True))
        out["warp_best_ms"] = min(t_warp)
        out["encode_over_warp"] = best["all"] / min(t_warp)
        try:
            from PIL import Image
            im = Image.fromarray(pic)
            cpu = []
            for _ in range(3):
                t0 = time.perf_counter()
                b = io.BytesIO()
                im.save(b, "JPEG", quality=quality, subsampling=0, optimize=False)
                cpu.append(1e3 * (time.perf_counter() - t0))
            out["pil_best_ms"], out["pil_bytes"] = min(cpu), len(b.getvalue())
            out["pil_over_encode"] = min(cpu) / best["all"]
        except ImportError:
            out["pil_best_ms"] = None
        with tempfile.TemporaryDirectory() as td:
            host, plain = [], []
            for k in range(3):
                t0 = time.perf_counter()
                J.write(Path(td) / f"{k}.jpg", pic, quality)
                host.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                with open(Path(td) / f"{k}.ppm", "wb") as f:
                    f.write(b"P%d\n%d %d\n255\n" % (6 if planes == 3 else 5, w, h))
                    f.write(pic.tobytes())
                plain.append(1e3 * (time.perf_counter() - t0))
            out["host_jpg_best_ms"], out["host_pnm_best_ms"] = min(host), min(plain)
        results.append(out)
        print(json.dumps(out), flush=True)
    return results


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gpu"])
    ap.add_argument("--sizes", default="1568x1440x1,2784x1440x3,8192x4096x3")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--only-encode", action="store_true")
    a = ap.parse_args()
    gpu([tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")], a.quality, a.reps, not a.no_check, a.only_encode)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
