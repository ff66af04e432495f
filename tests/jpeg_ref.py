"""A small baseline JPEG decoder in numpy, written from ITU-T T.81 and the JFIF specification, not from the encoder under test: the
markers are parsed and every table is taken from the file (B.2), the Huffman codes are generated from BITS and HUFFVAL (C.2, F.2.2.3),
the scan is decoded with its restart intervals (F.2.2, E.2.4), and the samples come from a float64 inverse transform (A.3.3) and the
JFIF colour equations.  It reads what the tests need: SOF0, 8 bit, one or three components without subsampling, one scan."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def dct_matrix() -> np.ndarray:
    """C[u][x] of the orthonormal 8-point DCT-II: F = C f C^T, f = C^T F C."""
    u, x = np.mgrid[0:8, 0:8]
    c = np.cos((2 * x + 1) * u * np.pi / 16) / 2
    c[0] /= np.sqrt(2)
    return c


@dataclass
class Jpeg:
    width: int = 0
    height: int = 0
    planes: int = 0
    restart_interval: int = 0
    jfif: tuple | None = None                  # (major, minor, units, x density, y density)
    qt: dict = field(default_factory=dict)     # table id -> uint16 [64], natural order (8 row + column)
    dht: dict = field(default_factory=dict)    # (class, id) -> (bits [16], vals)
    components: list = field(default_factory=list)   # (id, h, v, quantiser id)
    scan: list = field(default_factory=list)   # (component id, dc table, ac table)
    markers: list = field(default_factory=list)       # the marker bytes in the order met, RSTm included
    segments: int = 0
    stuffed: int = 0                           # 00 bytes taken out of the scan
    coef: np.ndarray | None = None             # int32 [mcus * planes, 64]: quantised, zig-zag order, the blocks of an MCU adjacent
    samples: np.ndarray | None = None          # float64 [H, W, planes]: Y, Cb, Cr (or grey) of the inverse transform, clamped, not rounded
    pixels: np.ndarray | None = None           # uint8 [H, W] or [H, W, 3]: grey or R, G, B


def _lookup(bits, vals):
    """For every 16-bit window the (symbol, length) of the code it begins with (length 0: none): the codes of C.2."""
    sym, size = np.zeros(65536, np.int32), np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(int(bits[length - 1])):
            lo = code << (16 - length)
            sym[lo: lo + (1 << (16 - length))] = vals[k]
            size[lo: lo + (1 << (16 - length))] = length
            code += 1
            k += 1
        code <<= 1
    return sym, size


class _Bits:
    def __init__(self, data: bytes):
        self.n = 8 * len(data)
        self.v = int.from_bytes(data + b"\xff\xff\xff\xff", "big")
        self.total = self.n + 32
        self.pos = 0

    def peek16(self) -> int:
        return (self.v >> (self.total - self.pos - 16)) & 0xFFFF

    def take(self, k: int) -> int:
        r = (self.v >> (self.total - self.pos - k)) & ((1 << k) - 1) if k else 0
        self.pos += k
        return r

    def symbol(self, table) -> int:
        w = self.peek16()
        length = int(table[1][w])
        if not length or self.pos + length > self.n:
            raise ValueError("no Huffman code at this place of the scan")
        self.pos += length
        return int(table[0][w])

    def extend(self, s: int) -> int:
        if self.pos + s > self.n:
            raise ValueError("the scan ends inside a value")
        v = self.take(s)
        return v if not s or v >= (1 << (s - 1)) else v - (1 << s) + 1       # F.2.2.1 EXTEND


def decode(data: bytes, pixels: bool = True) -> Jpeg:
    data = bytes(data)
    j = Jpeg()
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    j.markers.append(0xD8)
    p, scan_at = 2, None
    while scan_at is None:
        if data[p] != 0xFF:
            raise ValueError(f"no marker at byte {p}")
        m = data[p + 1]
        n = int.from_bytes(data[p + 2: p + 4], "big")
        body = data[p + 4: p + 2 + n]
        if len(body) != n - 2:
            raise ValueError("a marker segment runs past the file")
        j.markers.append(m)
        if m == 0xE0 and body[:5] == b"JFIF\0":
            j.jfif = (body[5], body[6], body[7], int.from_bytes(body[8:10], "big"), int.from_bytes(body[10:12], "big"))
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq:
                    raise ValueError("a 16-bit quantiser in a baseline file")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(body[q + 1: q + 65], np.uint8)
                j.qt[tq] = t
                q += 65
        elif m == 0xC0:
            if body[0] != 8:
                raise ValueError("not 8 bit")
            j.height, j.width, j.planes = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            j.components = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(j.planes)]
            if any(h != 1 or v != 1 for _, h, v, _ in j.components) or j.planes not in (1, 3):
                raise ValueError("subsampled components are not read here")
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise ValueError("not baseline (SOF0)")
        elif m == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                bits = np.frombuffer(body[q + 1: q + 17], np.uint8)
                count = int(bits.sum())
                j.dht[(tc, th)] = (bits.copy(), np.frombuffer(body[q + 17: q + 17 + count], np.uint8).copy())
                q += 17 + count
        elif m == 0xDD:
            j.restart_interval = int.from_bytes(body[:2], "big")
        elif m == 0xDA:
            ns = body[0]
            j.scan = [(body[1 + 2 * c], body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(ns)]
            if ns != j.planes or tuple(body[1 + 2 * ns: 4 + 2 * ns]) != (0, 63, 0):
                raise ValueError("one scan of all components, Ss 0, Se 63, Ah Al 0, is read here")
            scan_at = p + 2 + n
        p += 2 + n
    # ---- the scan: the intervals between the RSTm, the 00 bytes taken out (B.1.1.5, E.2.4)
    parts, cur, p = [], bytearray(), scan_at
    while True:
        b = data[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
            continue
        nxt = data[p + 1]
        if nxt == 0:
            cur.append(0xFF)
            j.stuffed += 1
            p += 2
        elif 0xD0 <= nxt <= 0xD7:
            if nxt - 0xD0 != len(parts) % 8:
                raise ValueError(f"RST{nxt - 0xD0} where RST{len(parts) % 8} is due")
            j.markers.append(nxt)
            parts.append(bytes(cur))
            cur = bytearray()
            p += 2
        elif nxt == 0xD9:
            j.markers.append(nxt)
            parts.append(bytes(cur))
            if p + 2 != len(data):
                raise ValueError("bytes behind EOI")
            break
        else:
            raise ValueError(f"marker FF {nxt:02X} inside the scan")
    mx, my = (j.width + 7) // 8, (j.height + 7) // 8
    n_mcus = mx * my
    ri = j.restart_interval or n_mcus
    if len(parts) != (n_mcus + ri - 1) // ri:
        raise ValueError(f"{len(parts)} intervals for {n_mcus} MCUs of {ri}")
    j.segments = len(parts)
    tables = {k: _lookup(*v) for k, v in j.dht.items()}
    coef = np.zeros((n_mcus * j.planes, 64), np.int32)
    blk = 0
    for s, part in enumerate(parts):
        r = _Bits(part)
        pred = [0] * j.planes
        for _ in range(min(ri, n_mcus - s * ri)):
            for c in range(j.planes):
                _, td, ta = j.scan[c]
                row = coef[blk]
                pred[c] += r.extend(r.symbol(tables[(0, td)]))
                row[0] = pred[c]
                k = 1
                while k < 64:
                    rs = r.symbol(tables[(1, ta)])
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run == 15:
                            k += 16
                            continue
                        if run == 0:
                            break
                        raise ValueError("an EOBn in a sequential scan")
                    k += run
                    if k > 63:
                        raise ValueError("a run past the end of a block")
                    row[k] = r.extend(size)
                    k += 1
                if k > 64:
                    raise ValueError("a ZRL past the end of a block")
                blk += 1
        left = r.n - r.pos
        if left >= 8 or r.take(left) != (1 << left) - 1:
            raise ValueError(f"interval {s} ends with {left} bits that are no padding of 1-bits")
    j.coef = coef
    if pixels:
        c = dct_matrix()
        out = np.zeros((my * 8, mx * 8, j.planes))
        qs = [j.qt[tq].astype(np.float64) for _, _, _, tq in j.components]
        nat = np.zeros((n_mcus, j.planes, 64))
        nat[:, :, ZIGZAG] = coef.reshape(n_mcus, j.planes, 64)
        for k in range(j.planes):
            f = (nat[:, k, :] * qs[k]).reshape(n_mcus, 8, 8)
            s = np.einsum("ux,nuv,vy->nxy", c, f, c) + 128.0                 # f = C^T F C
            out[:, :, k] = s.reshape(my, mx, 8, 8).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)
        j.samples = np.clip(out[: j.height, : j.width], 0.0, 255.0)          # A.3.1: a sample outside 0 .. 255 is clamped
        if j.planes == 1:
            j.pixels = np.clip(np.floor(j.samples[:, :, 0] + 0.5), 0, 255).astype(np.uint8)
        else:
            y, cb, cr = j.samples[:, :, 0], j.samples[:, :, 1] - 128.0, j.samples[:, :, 2] - 128.0
            rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=2)
            j.pixels = np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)
    return j


def entropy_only(segments: bytes, n_mcus: int, planes: int, restart_interval: int, dht: dict) -> np.ndarray:
    """The coefficients of bare segments (no head, no EOI) under the given tables: a minimal file is put around them."""
    head = bytearray(b"\xff\xd8")
    head += b"\xff\xdb" + (2 + 65).to_bytes(2, "big") + b"\0" + bytes([1] * 64)
    if planes == 3:
        head += b"\xff\xdb" + (2 + 65).to_bytes(2, "big") + b"\1" + bytes([1] * 64)
    mx = next(k for k in range(min(n_mcus, 8191), 0, -1) if n_mcus % k == 0)     # a picture of mx x my MCUs, both within 16 bits of pixels
    head += b"\xff\xc0" + (8 + 3 * planes).to_bytes(2, "big") + b"\x08" + (8 * (n_mcus // mx)).to_bytes(2, "big") + (8 * mx).to_bytes(2, "big") + bytes([planes])
    for c in range(planes):
        head += bytes([c + 1, 0x11, 1 if c else 0])
    for (tc, th), (bits, vals) in dht.items():
        head += b"\xff\xc4" + (2 + 17 + len(vals)).to_bytes(2, "big") + bytes([(tc << 4) | th]) + bytes(bits.tolist()) + bytes(vals.tolist())
    head += b"\xff\xdd\x00\x04" + restart_interval.to_bytes(2, "big")
    head += b"\xff\xda" + (6 + 2 * planes).to_bytes(2, "big") + bytes([planes])
    for c in range(planes):
        head += bytes([c + 1, 0x11 if c else 0x00])
    head += b"\x00\x3f\x00"
    return decode(bytes(head) + segments + b"\xff\xd9", pixels=False).coef
