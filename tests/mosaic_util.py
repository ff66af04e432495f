"""The blend of include/meteor_demod_amd_mosaic.h in vectorised int64 numpy, written from the header's text next to
map_util.warp_reference, and the hand-made passes the CPU and GPU tests share.  Nothing here calls the library."""
from __future__ import annotations

import functools

import numpy as np

import map_util as MU
import picture_util as PU

FEATHER, BEST = 0, 1
SIZES = ((4, 1), (36, 150), (200, 150))        # (width, height): the output sizes for which map_util.warp_cases has several cases


def blend_reference(sources, select, width: int, height: int, blend: int):
    """``sources``: a list of (images, filled, luts [planes, 256], nodes) or None.  (uint8 [height, width, planes], valid, cover): with BEST the cover
    holds the passes whose byte was taken."""
    i, j = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    a, b, p, q = i >> 4, j >> 4, i & 15, j & 15
    wq = [(16 - p) * (16 - q), p * (16 - q), (16 - p) * q, p * q]
    planes = len(select)
    num, den = np.zeros((height, width, planes), dtype=np.int64), np.zeros((height, width, planes), dtype=np.int64)
    cover, best = np.zeros((height, width), dtype=np.uint8), np.zeros((height, width, planes), dtype=np.int64)

    def rule(fa, fb, va, vb, f):
        return np.where(fa & fb, (va * (256 - f) + vb * f + 128) >> 8, np.where(fa, va, vb)), fa | fb
    for k, src in enumerate(sources):
        if src is None:
            continue
        images, filled, luts, nodes = src
        rows = next(x for x in images if x is not None).shape[0] // 8
        n = np.asarray(nodes, dtype=np.int64)
        corners = [n[a, b], n[a + 1, b], n[a, b + 1], n[a + 1, b + 1]]
        there = np.ones(i.shape, dtype=bool)
        for c in corners:
            there &= ~((c[..., 0] == MU.NO_NODE) & (c[..., 1] == MU.NO_NODE))
        X = (sum(wq[m] * corners[m][..., 0] for m in range(4)) + 128) >> 8
        Y = (sum(wq[m] * corners[m][..., 1] for m in range(4)) + 128) >> 8
        last = 8 * rows - 1
        inside = there & (X >= 0) & (X <= 1567 * 256) & (Y >= 0) & (Y <= last * 256)
        X, Y = np.where(inside, X, 0), np.where(inside, Y, 0)
        w = 1 + (np.minimum(np.minimum(X, 1567 * 256 - X), np.minimum(Y, last * 256 - Y)) >> 8)
        ix, fx, iy, fy = X >> 8, X & 255, Y >> 8, Y & 255
        ix2, iy2 = np.minimum(ix + 1, 1567), np.minimum(iy + 1, last)
        for pl, s in enumerate(select):
            im, cells = np.asarray(images[s], dtype=np.int64), np.asarray(filled[s]) != 0
            v0, c0 = rule(cells[iy // 8, ix // 112], cells[iy // 8, ix2 // 112], im[iy, ix], im[iy, ix2], fx)
            v1, c1 = rule(cells[iy2 // 8, ix // 112], cells[iy2 // 8, ix2 // 112], im[iy2, ix], im[iy2, ix2], fx)
            v, c = rule(c0, c1, v0, v1, fy)
            c &= inside
            byte = np.asarray(luts[pl], dtype=np.int64)[np.where(c, v, 0)]
            if blend == FEATHER:
                num[..., pl] += np.where(c, w * byte, 0)
                den[..., pl] += np.where(c, w, 0)
                cover |= c.astype(np.uint8) << k
            else:
                better = c & (w > den[..., pl])
                num[..., pl] = np.where(better, byte, num[..., pl])
                den[..., pl] = np.where(better, w, den[..., pl])
                best[..., pl] = np.where(better, k, best[..., pl])
    counted = den > 0
    if blend == BEST:
        for pl in range(planes):
            cover |= np.where(counted[..., pl], 1 << best[..., pl], 0).astype(np.uint8)
    safe = np.where(counted, den, 1)
    out = np.where(counted, (num + (safe >> 1)) // safe if blend == FEATHER else num, 0).astype(np.uint8)
    valid = np.zeros((height, width), dtype=np.uint8)
    for pl in range(planes):
        valid |= counted[..., pl].astype(np.uint8) << pl
    return out, valid, cover


@functools.lru_cache(maxsize=None)
def pass_data(kind: str, rows: int, seed: int):
    """(images, filled, luts [3, 256]) of one hand-made pass: random bytes under the masks of ``kind``."""
    return PU.pixels(rows, 31 + seed), PU.masks(kind, rows, 4 + seed), PU.random_luts(2 + seed)


@functools.lru_cache(maxsize=None)
def node_grids(width: int, height: int) -> list:
    """Node grids of one output size: the cases of map_util.warp_cases with that size, then affine grids that overlap each other
    (shifted, sheared, one half a pixel off), a grid of any int32 and one with all nodes missing.  At least 8."""
    rng = np.random.default_rng(1000 * width + height)
    grids = [nodes for _, w, h, nodes in MU.warp_cases() if (w, h) == (width, height)]
    grids.append(MU.affine_nodes(width, height, lambda i, j: 256 * (j + 700) + 100, lambda i, j: 200 * i + 13))
    grids.append(MU.affine_nodes(width, height, lambda i, j: 300 * j + 40 * i + 256 * 1400, lambda i, j: 256 * 10 - 30 * j + 90 * i))
    grids.append(MU.affine_nodes(width, height, lambda i, j: 256 * (j + 760) + 128, lambda i, j: 128 * i + 128))
    shape = MU.nodes_shape(width, height)
    wild = rng.integers(-(1 << 31) + 1, 1 << 31, shape, dtype=np.int64)
    near = rng.random(shape[:2]) < 0.7
    wild[near] = rng.integers(-3000, 1600 * 256, (int(near.sum()), 2))
    wild[..., 1][near] = rng.integers(-500, 45 * 256, int(near.sum()))
    grids.append(wild.astype(np.int32))
    grids.append(np.full(shape, MU.NO_NODE, dtype=np.int32))
    grids.append(MU.affine_nodes(width, height, lambda i, j: 256 * (1567 - j) - 17 * i, lambda i, j: 256 * 20 - 100 * i))
    holes = MU.affine_nodes(width, height, lambda i, j: 256 * (j + 5), lambda i, j: 256 * i + 77)
    holes[rng.random(shape[:2]) < 0.15] = MU.NO_NODE
    grids.append(holes)
    grids.append(MU.affine_nodes(width, height, lambda i, j: 64 * j + 256 * 783, lambda i, j: 64 * i + 256 * 3))
    assert len(grids) >= 8
    return grids


def sources(kind: str, width: int, height: int, n: int, planes: int) -> list:
    """``n`` hand-made passes on one output size: passes of 3 and 5 strip rows in turn, each with data and tables of its own; the
    all-missing grid is among the first three."""
    grids = node_grids(width, height)
    missing = next(k for k, g in enumerate(grids) if (g == MU.NO_NODE).all())
    order = [k for k in range(len(grids)) if k != missing]
    order.insert(2, missing)
    out = []
    for k in range(n):
        images, filled, luts = pass_data(kind, 3 if k % 2 == 0 else 5, k)
        out.append((images, filled, luts[:planes], grids[order[k % len(order)]]))
    return out
