"""Rates of the PNG encoder (include/meteor_demod_amd_png.h); numbers go to profiles/png.md.

    python tools/png_rate.py gpu [--reps 5] [--sizes 1568x1440x1,2784x1440x3,8192x4096x3]
        per size, inside one process: mdemod_png_encode_device on a synthetic picture in device memory (smooth ground, edges, noise of
        sigma 6, a black no-data border of about 40 %) between two device events, `reps` calls after a warm-up, without and with the
        border as a mask; the deflate stage alone on the same filtered bytes (mdemod_png_deflate_device: png_deflate, png_offsets,
        png_place) and once more with out_room 0, where png_place returns at once; the filter is the difference.  Beside them, for the
        same picture: a device-to-device copy, mdemod_map_warp_device making a picture of the same size, the JPEG encoder at quality
        90, PIL's PNG writer on one CPU core where PIL imports, and the host path: mdemod_png_encode_host plus writing the .png
        against writing the same pixels as a binary P5 / P6 file.  The file is checked against the host model byte for byte first.
    python tools/png_rate.py gpu --only-encode --no-check --sizes 8192x4096x3
        the calls of mdemod_png_encode_device alone: what a kernel trace of the four kernels is taken on, one size a process.
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

HBM_GB_PER_S = 8000.0


def the_picture(w: int, h: int, planes: int) -> tuple:
    """(picture, valid): the picture of tools/jpeg_rate.py inside a black border; valid is 0 on the border."""
    rng = np.random.default_rng(w + h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 128 + 70 * np.sin(xx / 37.0) * np.cos(yy / 51.0) + 40 * np.sin((xx + 2 * yy) / 230.0) + 30 * ((xx // 130 + yy // 90) % 2)
    if planes == 1:
        pic = np.clip(base + rng.normal(0, 6, (h, w)), 1, 255).astype(np.uint8)
    else:
        pic = np.clip(np.stack([base, 0.8 * base + 30, 255 - base], axis=2) + rng.normal(0, 6, (h, w, 3)), 1, 255).astype(np.uint8)
    inside = (np.abs(xx - w / 2) < w * 0.39) & (np.abs(yy - h / 2) < h * 0.39)
    pic[~inside] = 0
    return pic, inside.astype(np.uint8)


def gpu(sizes, reps: int, check: bool, only_encode: bool = False) -> list:
    import ctypes as C
    import torch
    from meteor_demod_amd import png as P
    assert torch.cuda.is_available(), "png_rate.py gpu needs a GPU"
    st = lambda: C.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def timed(fn, n=reps):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return times

    results = []
    for w, h, planes in sizes:
        pic, valid = the_picture(w, h, planes)
        d_pic, d_valid = torch.from_numpy(pic).cuda(), torch.from_numpy(valid).cuda()
        out = dict(width=w, height=h, planes=planes, reps=reps)
        t0 = time.perf_counter()
        got = P.encode_tensor(d_pic)
        out["first_call_ms"] = 1e3 * (time.perf_counter() - t0)
        out["file_bytes"], out["picture_bytes"] = len(got), pic.size
        if check:
            t0 = time.perf_counter()
            want = P.model_encode(pic)
            out["model_ms"] = 1e3 * (time.perf_counter() - t0)
            assert got == want, "the file differs from the model"
            assert P.encode_tensor(d_pic, d_valid) == P.model_encode(pic, valid), "the file with a mask differs from the model"
        room = P.bound(w, h, planes, True)
        need = P.workspace(w, h, planes, True)
        d_out = torch.empty(room, dtype=torch.uint8, device="cuda")
        d_work = torch.empty(need, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(2, dtype=torch.int64, device="cuda")

        def enc(mask):
            return P.lib().mdemod_png_encode_device(C.c_void_p(d_pic.data_ptr()), C.c_void_p(d_valid.data_ptr()) if mask else None, w, h, planes, 5, 0, C.c_void_p(d_out.data_ptr()),
                                                    room, C.c_void_p(d_res.data_ptr()), C.c_void_p(d_work.data_ptr()), need, 0, st())
        t_mask = timed(lambda: enc(True))
        out["file_bytes_with_mask"] = int(d_res.cpu()[0])
        t_all = timed(lambda: enc(False))
        assert d_out[: len(got)].cpu().numpy().tobytes() == got
        if only_encode:
            out["ms"] = dict(all=t_all, all_with_mask=t_mask)
            results.append(out)
            print(json.dumps(out), flush=True)
            continue
        # the filtered stream lies at the head of the workspace: the deflate stage alone, with a workspace of its own
        n_f = h * (1 + w * planes)
        d_f = d_work[:n_f].clone()
        need2 = int(P.lib().mdemod_png_deflate_workspace(n_f, 0))
        d_work2 = torch.empty(need2, dtype=torch.uint8, device="cuda")
        dfl = lambda r: P.lib().mdemod_png_deflate_device(C.c_void_p(d_f.data_ptr()), n_f, 0, C.c_void_p(d_out.data_ptr()), r, C.c_void_p(d_res.data_ptr()),
                                                          C.c_void_p(d_work2.data_ptr()), need2, 0, st())
        t_dfl, t_noplace = timed(lambda: dfl(room)), timed(lambda: dfl(0))
        segs = -(-n_f // 32768)
        best = dict(all=min(t_all), all_with_mask=min(t_mask), deflate_stage=min(t_dfl), deflate_and_offsets=min(t_noplace))
        best["filter"] = best["all"] - best["deflate_stage"]
        best["place"] = best["deflate_stage"] - best["deflate_and_offsets"]
        out["ms"] = dict(all=t_all, all_with_mask=t_mask, deflate_stage=t_dfl, deflate_and_offsets=t_noplace)
        out["best_ms"] = best
        # bytes over the memory interface, read from the code: the filter reads every row twice (itself and as the row above) and once
        # more for filter 5 when the row is wider than a tile; the deflate stage reads the stream and writes the chunks into slots
        moved = dict(filter=(3 if w > 1024 else 2) * pic.size + n_f, deflate_and_offsets=n_f + len(got) + segs * 24, place=2 * len(got))
        out["bytes"] = moved
        out["gb_per_s"] = {k: moved[k] / best[k] / 1e6 for k in moved if best[k] > 0}
        out["share_of_8_tb_per_s"] = {k: v / HBM_GB_PER_S for k, v in out["gb_per_s"].items()}
        out["segments"] = segs
        out["us_per_segment_wave"] = 1e3 * best["deflate_and_offsets"] / max(1, -(-segs // 512))            # 256 CUs x 2 blocks
        # yardsticks for the same picture
        d_copy = torch.empty_like(d_pic)
        out["copy_best_ms"] = min(timed(lambda: d_copy.copy_(d_pic)))
        try:
            import map_util as MU
            from meteor_demod_amd import jpeg as J, map as M
            rng = np.random.default_rng(1)
            rows = 600
            images = [torch.from_numpy(rng.integers(0, 256, (8 * rows, 1568), dtype=np.uint8)).cuda() for _ in range(3)]
            filled = [torch.from_numpy((rng.random((rows, 14)) < 0.9).astype(np.uint8)).cuda() for _ in range(3)]
            luts = torch.from_numpy(np.stack([np.arange(256, dtype=np.uint8)] * 3)).cuda()
            ww = (w + 3) // 4 * 4
            fx, fy = (1567 * 256) // ww, ((8 * rows - 1) * 256) // h
            nodes = torch.from_numpy(MU.affine_nodes(ww, h, lambda i, j: np.minimum(fx * j, 1567 * 256), lambda i, j: np.minimum(fy * i, (8 * rows - 1) * 256))).cuda()
            # (always the colour warp: three planes of that size, also beside a grey picture)
            out["warp_best_ms"] = min(timed(lambda: M.warp(images, filled, (2, 1, 0), luts, nodes, ww, h, valid=True)))
            jroom, jneed = J.bound(w, h, planes), J.workspace(w, h, planes)
            j_out = torch.empty(jroom, dtype=torch.uint8, device="cuda")
            j_work = torch.empty(jneed, dtype=torch.uint8, device="cuda")
            out["jpeg_best_ms"] = min(timed(lambda: J.lib().mdemod_jpeg_encode_device(C.c_void_p(d_pic.data_ptr()), w, h, planes, 90, 0, C.c_void_p(j_out.data_ptr()), jroom,
                                                                                      C.c_void_p(d_res.data_ptr()), C.c_void_p(j_work.data_ptr()), jneed, 0, st())))
            out["jpeg_bytes"] = int(d_res.cpu()[0])
            del j_out, j_work
        except ImportError as e:
            out["yardsticks_missing"] = str(e)
        try:
            from PIL import Image
            im = Image.fromarray(pic)
            cpu = []
            for _ in range(1 if pic.size > 30_000_000 else 3):
                t0 = time.perf_counter()
                b = io.BytesIO()
                im.save(b, "PNG")
                cpu.append(1e3 * (time.perf_counter() - t0))
            out["pil_best_ms"], out["pil_bytes"] = min(cpu), len(b.getvalue())
            out["pil_over_encode"] = min(cpu) / best["all"]
        except ImportError:
            out["pil_best_ms"] = None
        with tempfile.TemporaryDirectory() as td:
            host, plain = [], []
            for k in range(3):
                t0 = time.perf_counter()
                P.write(Path(td) / f"{k}.png", pic)
                host.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                with open(Path(td) / f"{k}.ppm", "wb") as f:
                    f.write(b"P%d\n%d %d\n255\n" % (6 if planes == 3 else 5, w, h))
                    f.write(pic.tobytes())
                plain.append(1e3 * (time.perf_counter() - t0))
            out["host_png_best_ms"], out["host_pnm_best_ms"] = min(host), min(plain)
        results.append(out)
        print(json.dumps(out), flush=True)
    return results


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gpu"])
    ap.add_argument("--sizes", default="1568x1440x1,2784x1440x3,8192x4096x3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--only-encode", action="store_true")
    a = ap.parse_args()
    gpu([tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")], a.reps, not a.no_check, a.only_encode)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
