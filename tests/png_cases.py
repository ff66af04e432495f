"""Shared inputs of the PNG tests: the pictures and masks of the round trips, the pictures of the size yardstick, and the crafted byte
arrays of the deflate stage.  Everything is seeded and cached; nobody changes what these functions return."""
from __future__ import annotations

import functools
import heapq

import numpy as np

SIZES = [(1, 1), (2, 1), (3, 5), (17, 23), (1568, 16), (2784, 8), (8192, 2)]          # width x height
RUN_LENGTHS = [1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 517, 4097]


@functools.lru_cache(maxsize=None)
def picture(width: int, height: int, planes: int, seed: int = 0) -> np.ndarray:
    """A slope with a little noise, a flat black lower right corner and a saturated stripe: every filter wins some row."""
    rng = np.random.default_rng(1000 * seed + 7 * width + height + planes)
    yy, xx = np.mgrid[0:height, 0:width]
    base = (xx * 3 + yy * 5 + seed * 11) % 256
    pic = np.stack([(base * (c + 1) + 40 * c + rng.integers(0, 3, base.shape)) % 256 for c in range(planes)], axis=2)
    pic[(yy * 3 > height * 2) & (xx * 2 > width)] = 0
    pic[yy % 7 == 3] = 255
    pic[yy % 11 == 5] = rng.integers(0, 256, (planes,))
    band = (yy % 13 >= 8) & (yy % 13 <= 10)                                   # noise on a level: the average of two neighbours is nearest
    pic[band] = (100 + rng.integers(0, 12, pic.shape))[band]
    for y in range(11, height, 13):                                           # a noisy row again: Up leaves nothing
        pic[y] = pic[y - 1]
    pic = pic.astype(np.uint8)
    pic.setflags(write=False)
    return pic if planes == 3 else pic[:, :, 0]


@functools.lru_cache(maxsize=None)
def mask(width: int, height: int, seed: int = 0) -> np.ndarray:
    """The map layer's kind of mask: 0 and non-zero values (not only 1), invalid in blobs and in single pixels."""
    rng = np.random.default_rng(77 + 1000 * seed + 3 * width + height)
    yy, xx = np.mgrid[0:height, 0:width]
    m = np.where((xx + 2 * yy) % 13 < 9, rng.integers(1, 256, (height, width)), 0)
    m[rng.random((height, width)) < 0.05] = 0
    m = m.astype(np.uint8)
    m.setflags(write=False)
    return m


def filtered_reference(pic: np.ndarray, valid, filt: int) -> np.ndarray:
    """The filtered stream by a numpy restatement of the header's rule: uint8 [height, 1 + width * channels]."""
    h, w = pic.shape[:2]
    px = pic.reshape(h, w, -1).astype(np.int32)
    if valid is not None:
        px = np.concatenate([px, np.where(np.asarray(valid) != 0, 255, 0)[:, :, None]], axis=2)
    ch = px.shape[2]
    rows = px.reshape(h, w * ch)
    zero_row = np.zeros(w * ch, np.int32)
    out = np.zeros((h, 1 + w * ch), np.uint8)
    for y in range(h):
        x = rows[y]
        b = rows[y - 1] if y else zero_row
        a = np.concatenate([np.zeros(ch, np.int32), x[:-ch]])
        c = np.concatenate([np.zeros(ch, np.int32), b[:-ch]])
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        cand = [x & 255, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth) & 255]
        if filt == 5:
            cost = [int(np.where(v < 128, v, 256 - v).sum()) for v in cand]
            f = int(np.argmin(cost))                                  # (the first of equal sums: the lower number)
        else:
            f = filt
        out[y, 0] = f
        out[y, 1:] = cand[f]
    return out


# --------------------------------------------------------------------------------------------------------- the size yardstick
@functools.lru_cache(maxsize=None)
def yardstick_pictures() -> dict:
    """512 lines x 1024 pixels: smooth, noise of sigma 2 and 8 on it, grey and colour, inside a black no-data border of about 40 %."""
    h, w = 512, 1024
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = 120 + 60 * np.sin(xx / 97.0) * np.cos(yy / 61.0) + 30 * np.sin((xx + 2 * yy) / 23.0)
    inside = (np.abs(xx - w / 2) < w * 0.39) & (np.abs(yy - h / 2) < h * 0.39)          # 0.78^2 = 61 % of the area
    out = {}
    for name, sigma in (("smooth", 0.0), ("noise2", 2.0), ("noise8", 8.0)):
        for planes in (1, 3):
            p = np.stack([smooth * (1 - 0.15 * c) + 10 * c + (rng.normal(0, sigma, smooth.shape) if sigma else 0) for c in range(planes)], axis=2)
            p = np.clip(np.rint(p), 0, 255).astype(np.uint8)
            p[~inside] = 0
            p.setflags(write=False)
            out[f"{name}_{'grey' if planes == 1 else 'colour'}"] = p if planes == 3 else p[:, :, 0]
    return out


# ------------------------------------------------------------------------------------------------------ crafted byte arrays
def _no_neighbours_equal(counts: dict) -> np.ndarray:
    """The symbols with these counts in an order in which no two equal ones are adjacent (the largest count is at most half)."""
    items = sorted(counts.items(), key=lambda kv: -kv[1])
    flat = np.concatenate([np.full(n, s, np.uint8) for s, n in items])
    out = np.zeros(flat.size, np.uint8)
    half = (flat.size + 1) // 2
    out[0::2], out[1::2] = flat[:half], flat[half:]
    assert (out[1:] != out[:-1]).all()
    return out


def huffman_depth(counts) -> int:
    """The depth of an unlimited Huffman code of these counts."""
    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


@functools.lru_cache(maxsize=None)
def crafted() -> dict:
    """name -> (bytes, segment in KiB)."""
    rng = np.random.default_rng(5)
    out = {}
    runs = [np.full(n, 10 + 3 * k, np.uint8) for k, n in enumerate(RUN_LENGTHS)]
    out["runs"] = (np.concatenate(runs), 32)
    out["runs_in_1k"] = (np.concatenate(runs), 1)                              # every long run is cut by segment starts as well
    a = (np.arange(3000) * 7 % 251).astype(np.uint8)
    a[1000:1100] = 77                                                          # a run across the segment start at 1024
    out["straddle"] = (a, 1)
    out["equal"] = (np.full(70000, 0, np.uint8), 32)                            # two full segments and a short one
    out["equal_ff"] = (np.full(2 * 1024 + 259, 255, np.uint8), 2)
    out["all256"] = (np.arange(256, dtype=np.uint8), 32)
    out["noise"] = (rng.integers(0, 256, 3 * 1024 + 100, dtype=np.uint8), 1)    # stored segments
    out["noise_then_flat"] = (np.concatenate([rng.integers(0, 256, 4096, dtype=np.uint8), np.zeros(4096, np.uint8)]), 4)
    out["last_of_one"] = (np.concatenate([(np.arange(1024) % 5).astype(np.uint8), np.array([9], np.uint8)]), 1)
    out["one_byte"] = (np.array([200], np.uint8), 32)
    out["two_bytes"] = (np.array([200, 200], np.uint8), 32)
    # counts that grow faster than Fibonacci's (c = the two before + 1): with the end-of-block's 1 every merge of a Huffman tree is
    # forced, whatever the tie order, and the code of these 18 symbols is 18 bits deep; 21 870 bytes, one segment
    fib = [1, 3]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2] + 1)
    out["skewed"] = (_no_neighbours_equal({20 + 5 * k: n for k, n in enumerate(fib)}), 32)
    # the same trouble for the code-length code: literal lengths 1, 2, 3 .. make every code-length symbol appear about once
    out["skewed_short"] = (_no_neighbours_equal({k: 2 ** k for k in range(9)}), 1)
    for v, _ in out.values():
        v.setflags(write=False)
    return out


def skewed_counts():
    a = crafted()["skewed"][0]
    return np.bincount(a, minlength=256).tolist() + [1]
