"""Test data of the sun layer, shared by the CPU and the GPU tests: two passes of the golden orbit chosen by date and onboard time
with sun_ref.py on the CPU (a daytime pass: every node below 70 degrees of zenith angle; a pass across the terminator: the smallest
below 80, the largest above 95), their packets, line times and gain tables, a synthetic table with missing nodes on every edge of a
cell, and random pictures that hold 0 and 255."""
from __future__ import annotations

import functools

import numpy as np

import map_ref as R
import map_util as M
import sun_ref as S

ROWS = 77                               # the passes are judged over this many strip rows


def _s0(u_deg: float) -> float:
    o = M.orbit()
    return o.epoch_sec + np.radians(u_deg) / o.u_dot + M.TIME_OFFSET


# name -> (days from the epoch's date, argument of latitude of line 0 in degrees, scan_deg).  The terminator pass has the widest scan
# short of missing nodes: at 110 degrees no 40 rows of a pass that reaches 95 degrees start below 71.8, which is 75 grey levels of the
# truth check's scene, and that check wants more than 100.
PASSES = {"day": (0, 150.0, 110.0), "terminator": (-75, 141.0, 122.0)}


def map_opts(name: str) -> dict:
    off, _, scan = PASSES[name]
    return dict(date=M.orbit().epoch_day + off, scan_deg=scan, time_offset=M.TIME_OFFSET)


def ref_pass(name: str, scan_deg: float | None = None) -> R.Pass:
    off, u, scan = PASSES[name]
    return R.Pass(M.orbit(), _s0(u), M.ROW_PERIOD, M.orbit().epoch_day + off, scan_deg=scan if scan_deg is None else scan_deg, time_offset=M.TIME_OFFSET)


@functools.lru_cache(maxsize=None)
def packets(name: str, rows: int = ROWS):
    return M.packets(rows, _s0(PASSES[name][1]))


def timing(name: str, rows: int = ROWS):
    from meteor_demod_amd import map as mp
    place, info = packets(name, rows)
    return mp.fit_time(place, info, **map_opts(name))


@functools.lru_cache(maxsize=None)
def ref_nodes(name: str, rows: int = ROWS, limit_deg: float = 85.0, ref_deg: float = 45.0, scan_deg: float | None = None):
    """sun_ref's (gain, unrounded gain, cos z) of the first ``rows`` strip rows of a pass; computed once, not to be changed."""
    out = S.nodes(ref_pass(name, scan_deg), rows, limit_deg, ref_deg)
    for a in out:
        a.setflags(write=False)
    return out


def synthetic_gain(rows: int, seed: int = 5) -> np.ndarray:
    """Gains 20 000 .. 2^22 - 1 with about every ninth node missing, and by hand a node missing on every edge of a cell: cell (0, 3)
    lacks only its upper left node, (0, 6) its upper right, (rows - 1, 9) its lower left, (rows - 1, 12) its lower right, and
    the last column and the last line of nodes, which lie one past the picture, lack one each."""
    rng = np.random.default_rng(seed + rows)
    g = rng.integers(20000, 1 << 22, (rows + 1, S.NODE_COLS), dtype=np.int64)
    g[rng.random(g.shape) < 0.11] = S.NO_NODE
    for a, b in ((0, 3), (0, 4), (1, 3), (1, 4), (0, 6), (0, 7), (1, 6), (1, 7), (rows - 1, 9), (rows - 1, 10), (rows, 9), (rows, 10), (rows - 1, 12), (rows - 1, 13),
                 (rows, 12), (rows, 13)):
        g[a, b] = 40000 + 1000 * b
    g[0, 3] = g[0, 7] = g[rows, 9] = g[rows, 13] = S.NO_NODE
    g[rows, 50] = g[rows // 2, 98] = S.NO_NODE
    g[0, 0] = (1 << 22) - 1
    g[0, 1], g[1, 0], g[1, 1] = (1 << 22) - 1, (1 << 22) - 1, (1 << 22) - 1          # the largest sum the header allows for
    return g.astype(np.uint32)


def gain_table(kind: str, rows: int) -> np.ndarray:
    """"day", "terminator" (sun_ref's table of the pass's first rows) or "synthetic"."""
    if kind == "synthetic":
        return synthetic_gain(rows)
    return np.array(ref_nodes(kind, rows)[0])


def pictures(rows: int, seed: int = 11) -> list:
    """Three random uint8 [8 rows, 1568] pictures; a share of the bytes is 0 and a share 255, and the first and the last pixel of
    every slot are 255 and 0."""
    rng = np.random.default_rng(seed + rows)
    out = []
    for k in range(3):
        p = rng.integers(0, 256, (8 * rows, S.WIDTH), dtype=np.uint8)
        r = rng.random(p.shape)
        p[r < 0.05] = 0
        p[r > 0.95] = 255
        p[0, 0], p[-1, -1] = 255, 0
        out.append(p)
    return out
