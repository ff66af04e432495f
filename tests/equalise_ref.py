"""A numpy model of the equalise layer, written from the opening comment of include/meteor_demod_amd_equalise.h alone (it is no
translation of csrc/equalise_host.cpp: whole-array operations, tile sums by slicing, the blend by fancy indexing).  Used by the CPU
and the GPU suite; also the pictures, masks and sizes both run over."""
from __future__ import annotations

import numpy as np


def channels_of(picture: np.ndarray, mode: int) -> np.ndarray:
    """int64 [channels, H, W]: the channel values of a picture [H, W] or [H, W, 3]."""
    p = picture.astype(np.int64)
    if p.ndim == 2 or p.shape[2] == 1:
        return p.reshape(1, p.shape[0], p.shape[1])
    if mode == 1:
        return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16)[None]
    return np.moveaxis(p, 2, 0).copy()


def counted_of(valid, h: int, w: int, valid_step: int) -> np.ndarray:
    if valid is None:
        return np.ones((h, w), bool)
    return np.repeat(np.asarray(valid) != 0, valid_step, axis=0)[:h]


def tiles_of(size: int, tile: int) -> int:
    return max(1, (size + tile // 2) // tile)


def edges_of(size: int, tile: int) -> list:
    n = tiles_of(size, tile)
    return [(t * tile, size if t == n - 1 else (t + 1) * tile) for t in range(n)]


def table_of(hist: np.ndarray, clip_percent: int) -> tuple:
    """(h'', tab) of one histogram (int64 [256])."""
    hist = hist.astype(np.int64)
    n = int(hist.sum())
    limit = max(1, (clip_percent * n + 25599) // 25600)
    excess = int(np.maximum(hist - limit, 0).sum())
    q, r = divmod(excess, 256)
    v = np.arange(256, dtype=np.int64)
    h2 = np.minimum(hist, limit) + q + ((v + 1) * r) // 256 - (v * r) // 256
    if n == 0:
        return h2, np.zeros(256, np.uint8)
    return h2, ((255 * np.cumsum(h2) + n // 2) // n).astype(np.uint8)


def tables(picture, valid=None, tile=128, clip_percent=300, mode=1, valid_step=1) -> tuple:
    """(tab uint8 [channels, ny, nx, 256], count uint32 [channels, ny, nx])."""
    picture = np.asarray(picture)
    h, w = picture.shape[:2]
    ch = channels_of(picture, mode)
    cnt = counted_of(valid, h, w, valid_step)
    ys, xs = edges_of(h, tile), edges_of(w, tile)
    tab = np.zeros((ch.shape[0], len(ys), len(xs), 256), np.uint8)
    count = np.zeros((ch.shape[0], len(ys), len(xs)), np.uint32)
    for c in range(ch.shape[0]):
        for ty, (y0, y1) in enumerate(ys):
            for tx, (x0, x1) in enumerate(xs):
                vals = ch[c, y0:y1, x0:x1][cnt[y0:y1, x0:x1]]
                hist = np.bincount(vals, minlength=256)
                count[c, ty, tx] = hist.sum()
                tab[c, ty, tx] = table_of(hist, clip_percent)[1]
    return tab, count


def _axis(size: int, tile: int, n: int) -> tuple:
    x = np.arange(size, dtype=np.int64)
    u = 2 * x + 1 - tile
    t0 = np.floor_divide(u, 2 * tile)
    f = u - 2 * tile * t0
    return np.maximum(t0, 0), np.minimum(t0 + 1, n - 1), f


def apply(picture, tab, count, valid=None, tile=128, amount=256, mode=1, valid_step=1) -> np.ndarray:
    picture = np.asarray(picture)
    h, w = picture.shape[:2]
    ch = channels_of(picture, mode)
    cnt = counted_of(valid, h, w, valid_step)
    ny, nx = tab.shape[1], tab.shape[2]
    ya, yb, fy = _axis(h, tile, ny)
    xa, xb, fx = _axis(w, tile, nx)
    new = np.zeros_like(ch)
    for c in range(ch.shape[0]):
        v = ch[c]
        S = np.zeros((h, w), np.int64)
        A = np.zeros((h, w), np.int64)
        for tyi, wy in ((ya, 2 * tile - fy), (yb, fy)):
            for txi, wx in ((xa, 2 * tile - fx), (xb, fx)):
                wgt = (wy[:, None] * wx[None, :]) * (count[c][tyi[:, None], txi[None, :]] != 0)
                S += wgt
                A += wgt * tab[c][tyi[:, None], txi[None, :], v].astype(np.int64)
        assert (S[cnt] > 0).all(), "the pixel's own tile is not empty"
        v1 = (A + S // 2) // np.maximum(S, 1)
        new[c] = (v * (256 - amount) + v1 * amount + 128) >> 8
    p = picture.astype(np.int64)
    if picture.ndim == 3 and picture.shape[2] == 3 and mode == 1:
        Y = ch[0][..., None]
        out = np.where(Y == 0, new[0][..., None], np.minimum(255, (p * new[0][..., None] + Y // 2) // np.maximum(Y, 1)))
    elif picture.ndim == 3:
        out = np.moveaxis(new, 0, 2)
    else:
        out = new[0]
    keep = cnt if picture.ndim == 2 else cnt[..., None]
    return np.where(keep, out, p).astype(np.uint8).reshape(picture.shape)


def equalise(picture, valid=None, tile=128, clip_percent=300, amount=256, mode=1, valid_step=1) -> tuple:
    """(out, tab, count)."""
    tab, count = tables(picture, valid, tile, clip_percent, mode, valid_step)
    return apply(picture, tab, count, valid, tile, amount, mode, valid_step), tab, count


# ---------------------------------------------------------------------------------------------- the cases of both suites
# (W, H, tile): the smallest picture; smaller than a tile, lines not on a dword; exactly one tile; a last tile of half a tile that is
# kept; a last tile that absorbs 7 columns and 7 rows; general; the largest tile with nx = 2, ny = 1; the widest row of tiles
SIZES = [(1, 1, 16), (7, 5, 16), (16, 16, 16), (40, 24, 16), (39, 23, 16), (300, 203, 16), (300, 203, 64), (1030, 67, 512), (8192, 16, 16)]
PICTURES = ["noise", "flat", "ramp", "two", "one"]
MASKS = ["none", "half", "gaps", "nothing", "step8"]
# (planes, mode)
LAYOUTS = [(1, 1), (3, 1), (3, 0)]


def picture_of(kind: str, w: int, h: int, planes: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng([seed, w, h, planes])
    shape = (h, w) if planes == 1 else (h, w, planes)
    if kind in ("noise", "one"):
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "flat":
        return np.full(shape, 77, np.uint8)
    if kind == "ramp":
        g = ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 5) % 256).astype(np.uint8)
        return g if planes == 1 else np.stack([g, 255 - g, (g // 2 + 60).astype(np.uint8)], axis=2)
    if kind == "two":
        g = np.where(rng.integers(0, 8, (h, w)) == 0, 200, 3).astype(np.uint8)
        return g if planes == 1 else np.stack([g, g, (255 - g).astype(np.uint8)], axis=2)
    raise ValueError(kind)


def mask_of(kind: str, picture_kind: str, w: int, h: int, tile: int, seed: int = 0) -> tuple:
    """(valid or None, valid_step).  The picture kind "one" leaves one counted pixel in every tile, whatever the mask kind (but
    "nothing")."""
    rng = np.random.default_rng([seed, w, h, 99])
    step = 8 if kind == "step8" else 1
    rows = (h + step - 1) // step
    if kind == "none":
        valid = None
    elif kind in ("half", "step8"):
        valid = (rng.integers(0, 2, (rows, w)) * 255).astype(np.uint8)
    elif kind == "gaps":
        valid = np.ones((rows, w), np.uint8)
        ys, xs = edges_of(h, tile), edges_of(w, tile)
        x0, x1 = xs[len(xs) // 2]
        y0, y1 = ys[len(ys) // 2]
        # a whole column and a whole row of tiles - where that would leave nothing at all, half of the picture instead
        if len(xs) > 1:
            valid[:, x0:x1] = 0
        if len(ys) > 1:
            valid[y0:y1, :] = 0
        if len(xs) == 1 and len(ys) == 1:
            valid[:, : w // 2] = 0
    elif kind == "nothing":
        valid = np.zeros((rows, w), np.uint8)
    else:
        raise ValueError(kind)
    if picture_kind == "one" and kind != "nothing":
        one = np.zeros((rows, w), np.uint8)
        for (y0, y1) in edges_of(h, tile):
            for (x0, x1) in edges_of(w, tile):
                one[int(rng.integers(y0, y1)) // step, int(rng.integers(x0, x1))] = 1
        valid, step = one, step
    return valid, step
