"""An independent numpy restatement of the picture layer (include/meteor_demod_amd_picture.h), written from the header's text: the
column map in float64, the contrast table and the render in int64, all vectorised.  The tests compare the library's host model
with it; nothing here calls the library."""
from __future__ import annotations

import numpy as np

R_EARTH, SRC_W, CELL_W, LAST = 6371.0, 1568, 112, 1567
OPTION_SETS = (dict(), dict(altitude_km=600.0, scan_deg=100.0), dict(altitude_km=900.0, scan_deg=114.0), dict(altitude_km=820.0, scan_deg=20.0))


def source_x(width: int, altitude_km: float = 820.0, scan_deg: float = 110.0) -> np.ndarray:
    """x(j) for j = 0 .. width - 1."""
    step = 2.0 * np.deg2rad(scan_deg / 2.0) / SRC_W
    g = (np.arange(width, dtype=np.float64) - (width - 1) / 2.0) * (altitude_km * step)
    return np.arctan2(R_EARTH * np.sin(g / R_EARTH), R_EARTH + altitude_km - R_EARTH * np.cos(g / R_EARTH)) / step + 783.5


def width_of(altitude_km: float = 820.0, scan_deg: float = 110.0) -> int:
    w = 4
    while source_x(w + 4, altitude_km, scan_deg)[0] >= 0.0:
        w += 4
    return w


def column_map(altitude_km: float = 820.0, scan_deg: float = 110.0, rectify: bool = True) -> np.ndarray:
    if not rectify:
        return (256 * np.arange(SRC_W)).astype(np.uint32)
    w = width_of(altitude_km, scan_deg)
    left = np.floor(256.0 * source_x(w, altitude_km, scan_deg)[: w // 2] + 0.5).astype(np.int64)
    return np.concatenate([left, (LAST * 256 - left)[::-1]]).astype(np.uint32)


def lut(hist, clip_low: int = 5, clip_high: int = 5):
    """(uint8 [256], lo, hi) by the header's rule."""
    h = np.asarray(hist, dtype=np.int64)
    n, cum = int(h.sum()), np.cumsum(h)
    identity = np.arange(256, dtype=np.uint8), 0, 255
    if n == 0:
        return identity
    before = np.concatenate([[0], cum[:-1]])
    lo = int(np.flatnonzero(1000 * cum > n * clip_low)[0])
    hi = int(np.flatnonzero(1000 * (n - before) > n * clip_high)[-1])
    if hi <= lo:
        return identity
    v = np.arange(256, dtype=np.int64)
    return np.minimum(np.maximum((v - lo) * 255 + (hi - lo) // 2, 0) // (hi - lo), 255).astype(np.uint8), lo, hi


def histogram(images, filled) -> np.ndarray:
    """uint32 [3, 256]: numpy.bincount over the pixels of the filled cells (a None slot stays zero)."""
    out = np.zeros((3, 256), dtype=np.uint32)
    for s in range(3):
        if images[s] is None:
            continue
        m = np.repeat(np.repeat(np.asarray(filled[s]) != 0, 8, axis=0), CELL_W, axis=1)
        out[s] = np.bincount(np.asarray(images[s])[m], minlength=256)
    return out


def render(images, filled, select, luts, cmap):
    """(uint8 [8 rows, W, planes], uint8 [rows, W])."""
    m = np.asarray(cmap, dtype=np.int64)
    i = np.minimum(m >> 8, LAST)
    f = m & 255
    i2 = np.minimum(i + 1, LAST)
    planes = len(select)
    lines = np.asarray(images[select[0]]).shape[0]
    out = np.zeros((lines, m.size, planes), dtype=np.uint8)
    valid = np.zeros((lines // 8, m.size), dtype=np.uint8)
    for p, s in enumerate(select):
        src = np.asarray(images[s], dtype=np.int64)
        cells = np.asarray(filled[s]) != 0
        a, b = src[:, i], src[:, i2]
        fa, fb = np.repeat(cells[:, i // CELL_W], 8, axis=0), np.repeat(cells[:, i2 // CELL_W], 8, axis=0)
        v = np.where(fa & fb, (a * (256 - f) + b * f + 128) >> 8, np.where(fa, a, b))
        out[:, :, p] = np.where(fa | fb, np.asarray(luts[p], dtype=np.uint8)[v], 0)
        valid |= ((fa | fb)[::8].astype(np.uint8) << p)
    return out, valid


def compose(images, filled, select, cmap=None, **opts):
    """The whole picture: (pixels, valid, [(lo, hi)]).  ``cmap``: a map to use in place of this module's own (the library's, where a
    test must not depend on the last bit of two atan2)."""
    stretch, cl, ch = opts.pop("stretch", True), opts.pop("clip_low", 5), opts.pop("clip_high", 5)
    cmap = column_map(**opts) if cmap is None else cmap
    hist = histogram(images, filled)
    tabs = [lut(hist[s], cl, ch) if stretch else (np.arange(256, dtype=np.uint8), 0, 255) for s in select]
    out, valid = render(images, filled, select, [t[0] for t in tabs], cmap)
    return out, valid, [(t[1], t[2]) for t in tabs]


# --------------------------------------------------------------------------------------------------------------- test data
def masks(kind: str, rows: int, seed: int = 0) -> list:
    """Three uint8 [rows, 14] masks: 'all', 'none', 'checker' (by cell: both one-tap cases at every cell border), 'empty1' (slot 1
    never received a strip), 'mixed' (every slot its own random mask)."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:rows, 0:14]
    if kind == "all":
        return [np.ones((rows, 14), np.uint8) for _ in range(3)]
    if kind == "none":
        return [np.zeros((rows, 14), np.uint8) for _ in range(3)]
    if kind == "checker":
        return [((r + c + s) % 2).astype(np.uint8) for s in range(3)]
    if kind == "empty1":
        return [np.ones((rows, 14), np.uint8), np.zeros((rows, 14), np.uint8), ((r + c) % 2).astype(np.uint8)]
    if kind == "mixed":
        return [rng.integers(0, 2, (rows, 14)).astype(np.uint8) * rng.integers(1, 256, (rows, 14)).astype(np.uint8) for _ in range(3)]
    raise ValueError(kind)


def pixels(rows: int, seed: int) -> list:
    """Three random uint8 [8 rows, 1568] pictures (unfilled cells hold garbage too: the mask decides, not the zeros)."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (8 * rows, SRC_W), dtype=np.uint8) for _ in range(3)]


def random_luts(seed: int = 1) -> np.ndarray:
    """uint8 [3, 256]: non-identity tables that reach 0 and 255."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8)

