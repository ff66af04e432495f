"""A float64 numpy model of include/meteor_demod_amd_polar.h, written from the header's text: the polar stereographic projection both
ways, the inverse of map_ref.Pass.forward by a two-dimensional Newton iteration in PROJECTED coordinates (the latitude / longitude
Newton of map_ref.inverse has no use near the pole, where a degree of longitude is no distance), and the bisection of the vertices.
It shares nothing with meteor_demod_amd/polar.py or csrc/polar_host.cpp."""
from __future__ import annotations

import math

import numpy as np

import map_ref as R

A, F = 6378137.0, 1.0 / 298.257223563
E2 = F * (2.0 - F)
E = math.sqrt(E2)


def t_of(phi):
    phi = np.asarray(phi, dtype=np.float64)
    return np.tan(np.pi / 4 - phi / 2) / ((1 - E * np.sin(phi)) / (1 + E * np.sin(phi))) ** (E / 2)


class Proj:
    """pole +1 / -1, lat_ts a magnitude in degrees, lon0 in degrees."""

    def __init__(self, pole: int, lat_ts_deg: float, lon0_deg: float):
        self.pole, self.lon0 = int(pole), float(lon0_deg)
        pc = math.radians(abs(lat_ts_deg))
        if abs(lat_ts_deg) == 90.0:
            self.scale = 2 * A / math.sqrt((1 + E) ** (1 + E) * (1 - E) ** (1 - E))
        else:
            self.scale = A * (math.cos(pc) / math.sqrt(1 - E2 * math.sin(pc) ** 2)) / float(t_of(pc))

    def forward(self, lat, lon):
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        rho = self.scale * t_of(np.radians(self.pole * lat))
        d = np.radians(lon - self.lon0)
        return rho * np.sin(d), -self.pole * rho * np.cos(d)

    def inverse(self, e, n):
        e, n = np.asarray(e, dtype=np.float64), np.asarray(n, dtype=np.float64)
        t = np.hypot(e, n) / self.scale
        phi = np.pi / 2 - 2 * np.arctan(t)
        for _ in range(10):
            nxt = np.pi / 2 - 2 * np.arctan(t * ((1 - E * np.sin(phi)) / (1 + E * np.sin(phi))) ** (E / 2))
            done = np.max(np.abs(nxt - phi), initial=0.0) < 1e-14
            phi = nxt
            if done:
                break
        lam = self.lon0 + np.degrees(np.arctan2(e, -self.pole * n))
        lam = np.where(np.hypot(e, n) == 0, self.lon0, lam)
        return self.pole * np.degrees(phi), (lam + 180.0) % 360.0 - 180.0


def margins(ref: R.Pass, lines: int):
    """(y_lo, y_hi, x_half): the edges of the margin in pixels."""
    per_line = ref.row_period / 8.0
    return -R.TIME_MARGIN / per_line, lines - 1 + R.TIME_MARGIN / per_line, (ref.scan_deg / 2 + R.SCAN_MARGIN) / (ref.scan_deg / 1568.0)


def inverse_pass(ref: R.Pass, proj: Proj, e, n, lines: int, steps: int = 14, seed=None):
    """The pixel (y, x) of ``ref`` that sees the point (e, n) of the plane, by Newton on project(forward(y, x)) from the nearest
    entry of a coarse table (or from ``seed`` = (y, x): only where the iteration starts); NaN where it does not converge to a
    millimetre or lies beyond the header's margin."""
    e, n = np.asarray(e, dtype=np.float64), np.asarray(n, dtype=np.float64)
    shape = e.shape
    e, n = e.reshape(-1), n.reshape(-1)
    y_lo, y_hi, x_half = margins(ref, lines)

    def plane(y, x):
        la, lo = ref.forward(y, x)
        with np.errstate(invalid="ignore"):
            return proj.forward(np.where(la * proj.pole > 0, la, np.nan), lo)
    ty, tx = np.meshgrid(np.arange(y_lo - 100, y_hi + 164, 64.0), np.arange(783.5 - x_half, 783.5 + x_half + 24, 24.0), indexing="ij")
    te, tn = plane(ty, tx)
    ok = np.isfinite(te)
    ty, tx, te, tn = ty[ok], tx[ok], te[ok], tn[ok]
    y, x = np.empty(e.size), np.empty(e.size)
    if seed is not None:
        y, x = (np.array(np.broadcast_to(np.asarray(s, dtype=np.float64), shape)).reshape(-1) for s in seed)
    for at in range(0, e.size if seed is None else 0, 2048):
        d = (e[at: at + 2048, None] - te[None]) ** 2 + (n[at: at + 2048, None] - tn[None]) ** 2
        best = np.argmin(d, axis=1)
        y[at: at + 2048], x[at: at + 2048] = ty[best], tx[best]
    good = np.zeros(e.size, dtype=bool)
    for _ in range(steps):
        pe, pn = plane(y, x)
        ey, ny = plane(y + 0.5, x)
        ex, nx = plane(y, x + 0.5)
        r0, r1 = e - pe, n - pn
        a, b, c, d = (ey - pe) / 0.5, (ex - pe) / 0.5, (ny - pn) / 0.5, (nx - pn) / 0.5
        det = a * d - b * c
        with np.errstate(invalid="ignore", divide="ignore"):
            dy, dx = (d * r0 - b * r1) / det, (-c * r0 + a * r1) / det
            good = np.isfinite(dy) & np.isfinite(dx) & (np.abs(r0) < 1e-3) & (np.abs(r1) < 1e-3)
        move = np.isfinite(dy) & np.isfinite(dx) & ~good
        y, x = np.where(move, y + np.clip(dy, -400, 400), y), np.where(move, x + np.clip(dx, -200, 200), x)
    inside = good & (y >= y_lo) & (y <= y_hi) & (np.abs(x - 783.5) <= x_half)
    return np.where(inside, y, np.nan).reshape(shape), np.where(inside, x, np.nan).reshape(shape)


def edge_distance(y, x, ref: R.Pass, lines: int):
    """Units of 1/256 pixel from (y, x) to the nearest edge of the margin."""
    y_lo, y_hi, x_half = margins(ref, lines)
    return 256.0 * np.minimum(np.minimum(np.abs(y - y_lo), np.abs(y - y_hi)), np.abs(np.abs(x - 783.5) - x_half))


# ------------------------------------------------------------------------------------------------------------------ vertices
def fixed(proj: Proj, frame, lon, lat):
    """Degrees to the overlay layer's fixed point on ``frame`` (anything with e_left, n_top, res), unrounded; plain floats through
    the math module."""
    phi = math.radians(proj.pole * lat)
    rho = proj.scale * math.tan(math.pi / 4 - phi / 2) / ((1 - E * math.sin(phi)) / (1 + E * math.sin(phi))) ** (E / 2)
    d = math.radians(lon) - math.radians(proj.lon0)
    e, n = rho * math.sin(d), -proj.pole * rho * math.cos(d)
    return 256.0 * ((e - frame.e_left) / frame.res - 0.5), 256.0 * ((frame.n_top - n) / frame.res - 0.5)


def wrap180(d: float) -> float:
    return (d + 180.0) % 360.0 - 180.0


def vertices(proj: Proj, frame, lon, lat, first, top: float = 64.0, levels: int = 12):
    """The header's bisection: (x, y, first) as lists of rounded integers."""
    xs, ys, firsts = [], [], []
    start = 0

    def close():
        nonlocal start
        if len(xs) - start >= 2:
            firsts.append(start)
        else:
            del xs[start:], ys[start:]
        start = len(xs)

    def between(a, pa, b, pb, level):
        if level >= levels:
            return
        m = (0.5 * (a[0] + b[0]), 0.5 * (a[1] + b[1]))
        pm = fixed(proj, frame, *m)
        if math.hypot(pm[0] - 0.5 * (pa[0] + pb[0]), pm[1] - 0.5 * (pa[1] + pb[1])) <= top:
            return
        between(a, pa, m, pm, level + 1)
        xs.append(math.floor(pm[0] + 0.5)); ys.append(math.floor(pm[1] + 0.5))
        between(m, pm, b, pb, level + 1)
    for l in range(len(first) - 1):
        prev = None
        for k in range(int(first[l]), int(first[l + 1])):
            if not lat[k] * proj.pole > 0:
                close()
                prev = None
                continue
            b = (float(lon[k]) if prev is None else prev[0][0] + wrap180(float(lon[k]) - prev[0][0]), float(lat[k]))
            pb = fixed(proj, frame, *b)
            if prev is not None:
                between(prev[0], prev[1], b, pb, 0)
            xs.append(math.floor(pb[0] + 0.5)); ys.append(math.floor(pb[1] + 0.5))
            prev = (b, pb)
        close()
    firsts.append(len(xs))
    return xs, ys, firsts
