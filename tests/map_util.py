"""Test data of the map layer: a synthetic sender's placements and time stamps with real timing (what the image layer reports for a
pass that loses nothing, or loses what the test says), a scene that is a function of latitude and longitude, and a painter that
samples it through the numpy forward function of map_ref.py into channel pictures."""
from __future__ import annotations

import functools

import numpy as np

import map_ref as R
from conftest import GOLDEN

PLACEMENT = np.dtype([("channel", "<i4"), ("row", "<u4"), ("cell", "<u4"), ("reserved", "<u4")])
STRIP_INFO = np.dtype([("mcus", "u1"), ("q", "u1"), ("mcun", "u1"), ("flags", "u1"), ("day", "<u2"), ("us", "<u2"), ("ms", "<u4"), ("bits_used", "<u4")])
ROW_PERIOD = 1.230769                   # a whole number of microseconds near 8 / 6.5 s: the stamps hold it without rounding
TIME_OFFSET = 10800.0


def tle_text() -> str:
    return (GOLDEN / "map_tle.txt").read_text()


@functools.lru_cache(maxsize=None)
def orbit() -> R.Orbit:
    return R.load(tle_text())


def second_set(norad: int = 99002, raan: float = 200.0) -> str:
    """The golden set under another catalogue number and another RAAN (checksums made right)."""
    name, l1, l2 = tle_text().splitlines()[:3]
    return "\n".join(["SYNTHETIC-M 2", R.edit(l1, 3, f"{norad:05d}"), R.edit(R.edit(l2, 3, f"{norad:05d}"), 18, f"{raan:8.4f}")]) + "\n"


def with_raan(raan: float) -> str:
    name, l1, l2 = tle_text().splitlines()[:3]
    return "\n".join([name, l1, R.edit(l2, 18, f"{raan % 360.0:8.4f}")]) + "\n"


def stamp(seconds):
    """Onboard seconds of the day to (ms, us) as the packets carry them."""
    total = np.rint(np.asarray(seconds, dtype=np.float64) * 1e6).astype(np.int64) % (86400 * 10 ** 6)
    return (total // 1000).astype(np.uint32), (total % 1000).astype(np.uint16)


def packets(rows: int, s0: float, period: float = ROW_PERIOD, keep=None, telemetry: bool = True):
    """(placements, reports) of a pass of ``rows`` strip rows: per row 14 packets of each of three channels and one that is not
    placed, every image packet of row r stamped s0 + r period.  ``keep``: bool [rows, 3, 14], the packets that arrive."""
    place, info = [], []
    ms, us = stamp(s0 + period * np.arange(rows))
    for r in range(rows):
        for ch in range(3):
            for c in range(14):
                if keep is None or keep[r, ch, c]:
                    place.append((ch, r, c, 0))
                    info.append((14, 60, 14 * c, 0, 7, us[r], ms[r], 900))
        if telemetry:
            place.append((-1, 0, 0, 0))
            info.append((0, 0, 0, 1, 0, 0, 0, 0))
    return np.array(place, dtype=PLACEMENT), np.array(info, dtype=STRIP_INFO)


def filled_of(place, rows: int) -> list:
    out = [np.zeros((rows, 14), dtype=np.uint8) for _ in range(3)]
    for ch, r, c, _ in place[place["channel"] >= 0]:
        out[ch][r, c] = 1
    return out


def mid_latitude_s0(first_u_deg: float = 15.0) -> float:
    """The onboard time at which the golden orbit stands ``first_u_deg`` degrees of argument of latitude past its ascending node
    (the node is at the epoch: omega + M = 360): a pass that starts there runs north over the middle latitudes."""
    o = orbit()
    return o.epoch_sec + np.radians(first_u_deg) / o.u_dot + TIME_OFFSET


def ref_pass(rows: int = 600, s0: float | None = None, text: str | None = None, **opts) -> R.Pass:
    o = orbit() if text is None else R.load(text)
    return R.Pass(o, mid_latitude_s0() if s0 is None else s0, ROW_PERIOD, o.epoch_day, time_offset=TIME_OFFSET, **opts)


# ----------------------------------------------------------------------------------------------------------------- the scene
MARKED_LEVEL = 128


def scene(lat, lon, channel: int, square: float, marked) -> np.ndarray:
    """Squares of ``square`` degrees in two grey levels, 64 and 192 (channel 1 the other way round), and level 128 in the square
    whose south-west corner is ``marked`` (lat, lon)."""
    a, b = np.floor(np.asarray(lat) / square).astype(np.int64), np.floor(np.asarray(lon) / square).astype(np.int64)
    level = np.where((a + b + (channel == 1)) % 2 == 0, 64, 192)
    here = (a == int(round(marked[0] / square))) & (b == int(round(marked[1] / square)))
    return np.where(here, MARKED_LEVEL, level).astype(np.uint8)


def edge_distance(lat, lon, square: float):
    """Degrees from (lat, lon) to the nearest edge of its square, in latitude and in longitude."""
    fa, fb = np.asarray(lat) / square, np.asarray(lon) / square
    return np.minimum(fa - np.floor(fa), np.ceil(fa) - fa) * square, np.minimum(fb - np.floor(fb), np.ceil(fb) - fb) * square


def paint(ref: R.Pass, rows: int, square: float, marked) -> list:
    """Three uint8 [8 rows, 1568] pictures: the scene at the footprint of every source pixel's centre."""
    y, x = np.meshgrid(np.arange(8.0 * rows), np.arange(1568.0), indexing="ij")
    lat, lon = ref.forward(y, x)
    assert np.isfinite(lat).all()
    return [scene(lat, lon, ch, square, marked) for ch in range(3)]


# ------------------------------------------------------------------------------------------------ hand-made node grids
NO_NODE = -(1 << 31)
SRC_ROWS = 3                            # the warp tests' source: 3 strip rows, 24 lines


def nodes_shape(width: int, height: int):
    return (-(-height // 16) + 1, -(-width // 16) + 1, 2)


def affine_nodes(width: int, height: int, x_of, y_of) -> np.ndarray:
    """Nodes of the affine map X = x_of(i, j), Y = y_of(i, j) in 1/256 source pixel.  The interpolation weights of a pixel sum to
    256, so an affine map with integer values at the nodes is reproduced exactly at every pixel."""
    a, b = np.meshgrid(16 * np.arange(nodes_shape(width, height)[0], dtype=np.int64), 16 * np.arange(nodes_shape(width, height)[1], dtype=np.int64), indexing="ij")
    return np.stack([x_of(a, b), y_of(a, b)], axis=-1).astype(np.int32)


def warp_cases() -> list:
    """(name, width, height, nodes): every way the warp can go, at sizes from 4 x 1 to 200 x 150 that include widths and heights
    which are no multiples of 16 or of a block's tile."""
    rng = np.random.default_rng(77)
    top = 8 * SRC_ROWS - 1
    cases = [
        ("identity", 200, 24, affine_nodes(200, 24, lambda i, j: 256 * (j + 700), lambda i, j: 256 * i)),
        ("identity, lines beyond the last", 36, 150, affine_nodes(36, 150, lambda i, j: 256 * j, lambda i, j: 256 * i)),
        ("half a pixel", 68, 17, affine_nodes(68, 17, lambda i, j: 256 * (j + 100) + 128, lambda i, j: 256 * i + 128)),
        ("magnified 8 times", 200, 150, affine_nodes(200, 150, lambda i, j: 32 * j + 111 * 256 - 7, lambda i, j: 32 * i + 5)),
        ("reduced 8 times", 196, 33, affine_nodes(196, 33, lambda i, j: 2048 * j + 3, lambda i, j: 181 * i)),
        ("rotated 90 degrees", 132, 150, affine_nodes(132, 150, lambda i, j: 256 * (i + 50) + 77, lambda i, j: 256 * top - 40 * j)),
        ("rotated 180 degrees", 200, 31, affine_nodes(200, 31, lambda i, j: 256 * (1567 - j), lambda i, j: 256 * top - 256 * i)),
        ("negative coordinates", 100, 40, affine_nodes(100, 40, lambda i, j: 256 * (j - 50) + 13, lambda i, j: 200 * (i - 9))),
        ("beyond the last column", 100, 20, affine_nodes(100, 20, lambda i, j: 256 * (j + 1500), lambda i, j: 256 * i + 31)),
        ("one pixel line", 4, 1, affine_nodes(4, 1, lambda i, j: 256 * (j + 111) + 200, lambda i, j: 256 * 7 + 255 + 0 * i)),
    ]
    missing = affine_nodes(200, 150, lambda i, j: 300 * j + 256 * 400, lambda i, j: 37 * i)
    missing[3, 5] = NO_NODE
    cases.append(("one node missing", 200, 150, missing))
    half = affine_nodes(52, 20, lambda i, j: 256 * j, lambda i, j: 256 * i)
    half[1, 1, 0] = NO_NODE                                                        # only one word: a node like any other
    cases.append(("one word of a node at the marker", 52, 20, half))
    cases.append(("all nodes missing", 72, 50, np.full(nodes_shape(72, 50), NO_NODE, dtype=np.int32)))
    wild = rng.integers(-(1 << 31) + 1, 1 << 31, nodes_shape(120, 90), dtype=np.int64)
    near = rng.random(nodes_shape(120, 90)[:2]) < 0.6
    wild[near] = rng.integers(-3000, 1600 * 256, (int(near.sum()), 2))
    wild[..., 1][near] = rng.integers(-500, 30 * 256, int(near.sum()))
    cases.append(("any int32 in the nodes", 120, 90, wild.astype(np.int32)))
    return cases


def warp_reference(images, filled, select, luts, nodes, width: int, height: int):
    """The header's warp in vectorised int64 numpy: (uint8 [height, width, planes], uint8 [height, width])."""
    rows = images[select[0]].shape[0] // 8
    i, j = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    n = np.asarray(nodes, dtype=np.int64)
    a, b, p, q = i >> 4, j >> 4, i & 15, j & 15
    corners = [n[a, b], n[a + 1, b], n[a, b + 1], n[a + 1, b + 1]]
    there = np.ones(i.shape, dtype=bool)
    for c in corners:
        there &= ~((c[..., 0] == NO_NODE) & (c[..., 1] == NO_NODE))
    # (int64: four weights that sum to 256 times an int32 stay below 2^40)
    w = [(16 - p) * (16 - q), p * (16 - q), (16 - p) * q, p * q]
    X = (sum(w[k] * corners[k][..., 0] for k in range(4)) + 128) >> 8
    Y = (sum(w[k] * corners[k][..., 1] for k in range(4)) + 128) >> 8
    last = 8 * rows - 1
    inside = there & (X >= 0) & (X <= 1567 * 256) & (Y >= 0) & (Y <= last * 256)
    X, Y = np.where(inside, X, 0), np.where(inside, Y, 0)
    ix, fx, iy, fy = X >> 8, X & 255, Y >> 8, Y & 255
    ix2, iy2 = np.minimum(ix + 1, 1567), np.minimum(iy + 1, last)
    out = np.zeros((height, width, len(select)), dtype=np.uint8)
    valid = np.zeros((height, width), dtype=np.uint8)

    def rule(fa, fb, va, vb, f):
        return np.where(fa & fb, (va * (256 - f) + vb * f + 128) >> 8, np.where(fa, va, vb)), fa | fb
    for pl, s in enumerate(select):
        src, cells = np.asarray(images[s], dtype=np.int64), np.asarray(filled[s]) != 0
        v0, c0 = rule(cells[iy // 8, ix // 112], cells[iy // 8, ix2 // 112], src[iy, ix], src[iy, ix2], fx)
        v1, c1 = rule(cells[iy2 // 8, ix // 112], cells[iy2 // 8, ix2 // 112], src[iy2, ix], src[iy2, ix2], fx)
        v, c = rule(c0, c1, v0, v1, fy)
        c &= inside
        out[..., pl] = np.where(c, np.asarray(luts[pl], dtype=np.uint8)[np.where(c, v, 0)], 0)
        valid |= c.astype(np.uint8) << pl
    return out, valid


# ------------------------------------------------------------------------------------------------------------ a recording
@functools.lru_cache(maxsize=1)
def recording():
    """image_util.recording() with real stamps: the same picture of one strip row, every image packet stamped with the onboard time
    of the mid-latitude pass's first row.  (Stream, s16 [n, 2])."""
    import frames_util as U
    import image_util as I
    from meteor_demod_amd import image
    pic = I.picture(3, I.PIC_ROWS)
    ms, us = stamp(mid_latitude_s0() + ROW_PERIOD * np.arange(I.PIC_ROWS))
    packets, seq = [], 100
    for r in range(I.PIC_ROWS):
        for k, apid in enumerate((64, 65, 66)):
            for c in range(14):
                packets.append(image.model_encode_packet(pic[k, 8 * r: 8 * r + 8, 112 * c: 112 * c + 112], I.PIC_Q, 14 * c, apid, seq & 0x3FFF, 7, int(ms[r]), int(us[r])))
                seq += 1
        packets.append(I.plain_packet(70, seq & 0x3FFF, 7 + 62, sec=1))
        seq += 1
    idle = [I.idle_packet(I.ZONE) for _ in range(I.LEAD_IDLE)]
    vcdus, _, _ = I.mux(idle + packets + [I.idle_packet(I.ZONE) for _ in range(I.TAIL_IDLE)])
    st = I.Stream(vcdus, seed=4243, lead=3000, tail=600)
    rng = np.random.default_rng(78)
    z = np.zeros(len(st.sym) * U.SPS, dtype=complex)
    z[::U.SPS] = st.sym[:, 0] + 1j * st.sym[:, 1]
    y = np.convolve(z, U._rrc(0.6, U.SPS, 8))
    y = y + np.sqrt(2 / 10 ** 1.3 / 2) * (rng.normal(size=len(y)) + 1j * rng.normal(size=len(y)))
    iq = np.stack([y.real, y.imag], axis=1) * 4000.0
    return st, np.clip(np.rint(iq), -32768, 32767).astype(np.int16)
