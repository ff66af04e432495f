"""A float64 numpy model of the orbit, time and look-vector section of include/meteor_demod_amd_map.h, written from the header's
text alone: it shares nothing with meteor_demod_amd/map.py or csrc/map_host.cpp but the TLE text.  Its inverse is a plain
two-dimensional Newton iteration on its own forward function, seeded from a coarse forward table."""
from __future__ import annotations

import datetime

import numpy as np

MU, RE, F, J2 = 398600.4418, 6378.137, 1.0 / 298.257223563, 1.08262668e-3
B, E2 = RE * (1.0 - F), F * (2.0 - F)
EARTH_RATE = np.radians(360.98564736629) / 86400.0          # rad / s
SCAN_MARGIN, TIME_MARGIN = 5.0, 120.0


def checksum(line: str) -> int:
    return sum(int(c) if c.isdigit() else 1 if c == "-" else 0 for c in line[:68]) % 10


def with_checksum(line: str) -> str:
    return line[:68] + str(checksum(line))


def edit(line: str, first: int, text: str) -> str:
    """``text`` written from column ``first`` (counted from 1) and the checksum made right again."""
    return with_checksum(line[: first - 1] + text + line[first - 1 + len(text):])


class Orbit:
    """The element set of the two lines ``l1`` and ``l2``."""

    def __init__(self, l1: str, l2: str):
        assert l1[0] == "1" and l2[0] == "2" and len(l1) == 69 and len(l2) == 69 and checksum(l1) == int(l1[68]) and checksum(l2) == int(l2[68])
        yy = int(l1[18:20])
        doy = float(l1[20:32])
        year = 2000 + yy if yy < 57 else 1900 + yy
        self.epoch_day = (datetime.date(year, 1, 1) - datetime.date(1970, 1, 1)).days + int(doy) - 1
        self.epoch_sec = (doy - int(doy)) * 86400.0
        self.norad = int(l1[2:7])
        self.inc, self.raan, self.argp, self.ma = (float(l2[a:b]) for a, b in ((8, 16), (17, 25), (34, 42), (43, 51)))
        self.ecc = float("0." + l2[26:33])
        self.mm = float(l2[52:63])
        n = self.mm * 2 * np.pi / 86400.0
        self.a = (MU / n ** 2) ** (1.0 / 3.0)
        k = 1.5 * J2 * (RE / self.a) ** 2 * n
        ci = np.cos(np.radians(self.inc))
        self.raan_dot = -k * ci
        self.u_dot = n + 0.5 * k * (5 * ci ** 2 - 1)

    def frame(self, date: int, sec):
        """r, v, h (each [..., 3]) in Earth-fixed coordinates at UTC second ``sec`` of day ``date``."""
        sec = np.asarray(sec, dtype=np.float64)
        dt = (date - self.epoch_day) * 86400.0 + (sec - self.epoch_sec)
        om = np.radians(self.raan) + self.raan_dot * dt
        u = np.radians(self.argp + self.ma) + self.u_dot * dt
        i = np.radians(self.inc)
        d = (date - 10957) + (sec - 43200.0) / 86400.0
        g = np.radians(np.mod(280.46061837 + 360.98564736629 * d, 360.0))
        r = np.stack([np.cos(om) * np.cos(u) - np.sin(om) * np.sin(u) * np.cos(i), np.sin(om) * np.cos(u) + np.cos(om) * np.sin(u) * np.cos(i),
                      np.sin(u) * np.sin(i)], axis=-1)
        v = np.stack([-np.cos(om) * np.sin(u) - np.sin(om) * np.cos(u) * np.cos(i), -np.sin(om) * np.sin(u) + np.cos(om) * np.cos(u) * np.cos(i),
                      np.cos(u) * np.sin(i)], axis=-1)
        h = np.cross(r, v)

        def fixed(w):
            return np.stack([w[..., 0] * np.cos(g) + w[..., 1] * np.sin(g), -w[..., 0] * np.sin(g) + w[..., 1] * np.cos(g), w[..., 2]], axis=-1)
        return fixed(r), fixed(v), fixed(h)


class Pass:
    """An orbit with line times: ``s0`` onboard seconds of line 0, ``row_period`` seconds per 8 lines, ``date`` days since 1970."""

    def __init__(self, orbit: Orbit, s0: float, row_period: float, date: int, scan_deg: float = 110.0, time_offset: float = 10800.0, side: int = 1):
        self.orbit, self.s0, self.row_period, self.date, self.scan_deg, self.time_offset, self.side = orbit, s0, row_period, date, scan_deg, time_offset, side
        self.step = np.radians(scan_deg / 1568.0)

    def sec(self, y):
        return self.s0 + np.asarray(y, dtype=np.float64) * self.row_period / 8.0 - self.time_offset

    def forward(self, y, x):
        """(lat, lon) in degrees of pixel (line y, column x); NaN where the pixel does not see the Earth."""
        y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
        r, _, h = self.orbit.frame(self.date, self.sec(y))
        th = (x - 783.5) * self.step
        look = -np.cos(th)[..., None] * r + self.side * np.sin(th)[..., None] * h
        sat = self.orbit.a * r
        w = np.array([1 / RE ** 2, 1 / RE ** 2, 1 / B ** 2])
        qa, qb, qc = (look * look * w).sum(-1), (sat * look * w).sum(-1), (sat * sat * w).sum(-1) - 1.0
        disc = qb ** 2 - qa * qc
        with np.errstate(invalid="ignore"):
            t = (-qb - np.sqrt(disc)) / qa
            t = np.where(t > 0, t, np.nan)
        p = sat + t[..., None] * look
        return np.degrees(np.arctan2(p[..., 2], (1 - E2) * np.hypot(p[..., 0], p[..., 1]))), np.degrees(np.arctan2(p[..., 1], p[..., 0]))

    def inverse(self, lat, lon, lines: int, steps: int = 12):
        """The pixel (y, x) that sees (lat, lon), by Newton on ``forward`` from the nearest entry of a coarse forward table; NaN
        where it does not converge to 1e-7 degree (1e-5 pixel), or the pixel lies beyond the margin of the header."""
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        shape = lat.shape
        lat, lon = lat.reshape(-1), lon.reshape(-1)
        per_line = self.row_period / 8.0
        y_lo, y_hi = -TIME_MARGIN / per_line, lines - 1 + TIME_MARGIN / per_line
        x_half = (self.scan_deg / 2 + SCAN_MARGIN) / (self.scan_deg / 1568.0)
        ty, tx = np.meshgrid(np.arange(y_lo - 100, y_hi + 164, 64.0), np.arange(783.5 - x_half, 783.5 + x_half + 24, 24.0), indexing="ij")
        tlat, tlon = self.forward(ty, tx)
        ok = np.isfinite(tlat)
        ty, tx, tlat, tlon = ty[ok], tx[ok], tlat[ok], tlon[ok]
        unit = lambda la, lo: np.stack([np.cos(np.radians(la)) * np.cos(np.radians(lo)), np.cos(np.radians(la)) * np.sin(np.radians(lo)), np.sin(np.radians(la))], -1)
        tu, pu = unit(tlat, tlon).astype(np.float32), unit(lat, lon).astype(np.float32)
        y, x = np.empty(lat.size), np.empty(lat.size)
        for at in range(0, lat.size, 4096):
            best = np.argmax(pu[at: at + 4096] @ tu.T, axis=1)
            y[at: at + 4096], x[at: at + 4096] = ty[best], tx[best]
        good = np.zeros(lat.size, dtype=bool)
        for _ in range(steps):
            la, lo = self.forward(y, x)
            la_y, lo_y = self.forward(y + 0.5, x)
            la_x, lo_x = self.forward(y, x + 0.5)
            wrap = lambda d: (d + 180.0) % 360.0 - 180.0
            e0, e1 = lat - la, wrap(lon - lo)
            a, b, c, d = (la_y - la) / 0.5, (la_x - la) / 0.5, wrap(lo_y - lo) / 0.5, wrap(lo_x - lo) / 0.5
            det = a * d - b * c
            with np.errstate(invalid="ignore", divide="ignore"):
                dy, dx = (d * e0 - b * e1) / det, (-c * e0 + a * e1) / det
            good = np.isfinite(dy) & np.isfinite(dx) & (np.abs(e0) < 1e-7) & (np.abs(e1) < 1e-7)
            move = np.isfinite(dy) & np.isfinite(dx) & ~good
            y, x = np.where(move, y + np.clip(dy, -400, 400), y), np.where(move, x + np.clip(dx, -200, 200), x)
        inside = good & (y >= y_lo) & (y <= y_hi) & (np.abs(x - 783.5) <= x_half)
        return np.where(inside, y, np.nan).reshape(shape), np.where(inside, x, np.nan).reshape(shape)


def load(text: str, norad: int = 0) -> Orbit:
    """The first set of a TLE text, or the one numbered ``norad``."""
    lines = [l.rstrip() for l in text.splitlines() if l.strip()]
    for a, b in zip(lines, lines[1:]):
        if a.startswith("1 ") and b.startswith("2 ") and (not norad or int(a[2:7]) == norad):
            return Orbit(a, b)
    raise ValueError("no element set")
