"""A numpy model of include/meteor_demod_amd_sun.h, written from the header's text alone: the sun's position, the cosine of its
zenith angle on map_ref.py's geolocation, the gain nodes of a pass, and the apply with its saturation counts in vectorised int64.
It shares nothing with meteor_demod_amd/sun.py or csrc/sun_host.cpp."""
from __future__ import annotations

import numpy as np

NO_NODE = 0xFFFFFFFF
NODE_COLS, WIDTH = 99, 1568


def position(date: int, utc):
    """The Earth-fixed unit vector(s) to the sun, [..., 3]."""
    utc = np.asarray(utc, dtype=np.float64)
    n = (date - 10957) + (utc - 43200.0) / 86400.0
    L = 280.460 + 0.9856474 * n
    g = np.radians(357.528 + 0.9856003 * n)
    lam = np.radians(L + 1.915 * np.sin(g) + 0.020 * np.sin(2 * g))
    eps = np.radians(23.439 - 0.0000004 * n)
    x, y, z = np.cos(lam), np.cos(eps) * np.sin(lam), np.sin(eps) * np.sin(lam)
    G = np.radians(np.mod(280.46061837 + 360.98564736629 * n, 360.0))
    return np.stack([x * np.cos(G) + y * np.sin(G), -x * np.sin(G) + y * np.cos(G), z], axis=-1)


def declination(date: int, utc: float) -> float:
    return float(np.degrees(np.arcsin(position(date, utc)[2])))


def subsolar_longitude(date: int, utc: float) -> float:
    s = position(date, utc)
    return float(np.degrees(np.arctan2(s[1], s[0])))


def cos_zenith(date: int, utc, lat, lon):
    s = position(date, utc)
    la, lo = np.radians(np.asarray(lat, dtype=np.float64)), np.radians(np.asarray(lon, dtype=np.float64))
    return s[..., 0] * np.cos(la) * np.cos(lo) + s[..., 1] * np.cos(la) * np.sin(lo) + s[..., 2] * np.sin(la)


def pass_cos_zenith(ref, y, x):
    """cos z at the footprint of pixel (line y, column x) of a map_ref.Pass at that line's time; NaN where it does not see the Earth."""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    lat, lon = ref.forward(y, x)
    return cos_zenith(ref.date, ref.sec(y), lat, lon)


def node_cos(ref, rows: int):
    a, b = np.meshgrid(np.arange(rows + 1), np.arange(NODE_COLS), indexing="ij")
    return pass_cos_zenith(ref, 8.0 * a, 16.0 * b)


def gain_of(c, limit_deg: float = 85.0, ref_deg: float = 45.0):
    """The real-valued gain 65536 cr / max(c, cl) before it is rounded."""
    return 65536.0 * np.cos(np.radians(ref_deg)) / np.maximum(c, np.cos(np.radians(limit_deg)))


def nodes(ref, rows: int, limit_deg: float = 85.0, ref_deg: float = 45.0):
    """(gain uint32 [rows + 1, 99], the unrounded 65536 gain (NaN where missing), cos z of the nodes)."""
    c = node_cos(ref, rows)
    real = gain_of(c, limit_deg, ref_deg)
    gain = np.where(np.isfinite(c), np.floor(np.where(np.isfinite(real), real, 0.0) + 0.5), NO_NODE).astype(np.uint32)
    return gain, real, c


def zenith_range(ref, rows: int) -> tuple:
    c = node_cos(ref, rows)
    z = np.degrees(np.arccos(np.clip(c[np.isfinite(c)], -1.0, 1.0)))
    return float(z.min()), float(z.max())


def pixel_gain(gain, rows: int):
    """(g int64 [8 rows, 1568], missing bool [8 rows, 1568]) of the header's interpolation."""
    G = np.asarray(gain, dtype=np.int64)
    y, x = np.meshgrid(np.arange(8 * rows), np.arange(WIDTH), indexing="ij")
    a, p, b, q = y >> 3, y & 7, x >> 4, x & 15
    c = [G[a, b], G[a + 1, b], G[a, b + 1], G[a + 1, b + 1]]
    missing = (c[0] == NO_NODE) | (c[1] == NO_NODE) | (c[2] == NO_NODE) | (c[3] == NO_NODE)
    g = ((8 - p) * (16 - q) * c[0] + p * (16 - q) * c[1] + (8 - p) * q * c[2] + p * q * c[3] + 64) >> 7
    return g, missing


def apply(images, gain, mask: int) -> tuple:
    """(three pictures - the slots that are not selected as given -, saturated [3]) for gain words below 2^22 or the marker."""
    rows = next(images[k].shape[0] // 8 for k in range(3) if mask >> k & 1)
    g, missing = pixel_gain(gain, rows)
    out, sat = list(images), [0, 0, 0]
    for k in range(3):
        if not (mask >> k & 1):
            continue
        v = np.asarray(images[k], dtype=np.int64)
        t = (v * g + 32768) >> 16
        sat[k] = int(np.count_nonzero((t > 255) & ~missing))
        out[k] = np.where(missing, v, np.minimum(t, 255)).astype(np.uint8)
    return out, sat
