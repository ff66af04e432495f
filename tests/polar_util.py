"""Test data of the polar layer: passes of the golden orbit near the top (and the bottom) of the orbit, the numpy references that go
with them, and the rule by which two node solvers agree (include/meteor_demod_amd_polar.h, "nodes")."""
from __future__ import annotations

import functools

import numpy as np

import map_util as MU
import polar_ref as PR

POLAR_U, SHORT_U, SOUTH_U = 60.0, 88.0, 230.0       # degrees of argument of latitude past the node at which the passes start
POLAR_ROWS, SHORT_ROWS = 600, 5                     # strip rows: 4800 lines, and the 40 lines that sit on the pole


def plain_pass(rows: int, s0: float, text: str | None = None):
    """A pass without pictures to speak of: what the grid entries look at."""
    from meteor_demod_amd import mosaic as M
    place, info = MU.packets(rows, s0)
    return M.Pass(MU.tle_text() if text is None else text, [np.zeros((8 * rows, 1568), np.uint8), None, None], [np.ones((rows, 14), np.uint8), None, None], place, info)


@functools.lru_cache(maxsize=None)
def polar_pass(first_u: float = POLAR_U, rows: int = POLAR_ROWS, raan: float | None = None, later: int = 0):
    """(pass, numpy pass)."""
    s0 = MU.mid_latitude_s0(first_u) + later * MU.ROW_PERIOD
    text = None if raan is None else MU.with_raan(raan)
    return plain_pass(rows, s0, text), MU.ref_pass(rows, s0=s0, text=text)


def proj_of(frame) -> PR.Proj:
    return PR.Proj(frame.pole, abs(frame.lat_ts_deg), frame.lon0_deg)


def node_centres(frame):
    """(E, N) of the output pixels (16 a, 16 b) the nodes stand for, each [node rows, node cols]."""
    rows, cols, _ = frame.nodes_shape
    a, b = np.meshgrid(16 * np.arange(rows), 16 * np.arange(cols), indexing="ij")
    return frame.centres(a, b)


def missing(nodes) -> np.ndarray:
    return (nodes[..., 0] == MU.NO_NODE) & (nodes[..., 1] == MU.NO_NODE)


def margin_edges(ref, lines: int):
    """The edges of the margin in units of 1/256 pixel: (Y low, Y high, X low, X high)."""
    y_lo, y_hi, x_half = PR.margins(ref, lines)
    return 256 * y_lo, 256 * y_hi, 256 * (783.5 - x_half), 256 * (783.5 + x_half)


def agreement(got, want, ref, lines: int):
    """The header's rule for two solvers of one pass's nodes.  (nodes that break it, nodes that differ at all, nodes)."""
    got, want = got.astype(np.int64), want.astype(np.int64)
    g_none, w_none = missing(got), missing(want)
    both = ~g_none & ~w_none
    close = both & (np.abs(got[..., 0] - want[..., 0]) <= 1) & (np.abs(got[..., 1] - want[..., 1]) <= 1)
    one = g_none ^ w_none
    there = np.where(g_none[..., None], want, got)
    y_lo, y_hi, x_lo, x_hi = margin_edges(ref, lines)
    near = (np.minimum(np.abs(there[..., 1] - y_lo), np.abs(there[..., 1] - y_hi)) <= 2) | (np.minimum(np.abs(there[..., 0] - x_lo), np.abs(there[..., 0] - x_hi)) <= 2)
    fine = (g_none & w_none) | close | (one & near)
    differ = one | (both & ((got[..., 0] != want[..., 0]) | (got[..., 1] != want[..., 1])))
    return int((~fine).sum()), int(differ.sum()), int(fine.size)
