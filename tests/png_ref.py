"""The tests' own PNG reader (standard library and numpy only), independent of csrc/png_host.h: chunks with every CRC checked by
``zlib.crc32``, the concatenated IDAT data inflated by ``zlib.decompressobj`` (which also proves the Adler-32), the filters undone."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def chunks(data: bytes, start: int = 8) -> list:
    """[(type, payload)] of the chunks from ``start`` on; every length and CRC is checked, and nothing may follow the last."""
    out, at = [], start
    while at < len(data):
        assert at + 12 <= len(data), "a chunk's frame runs past the end"
        n, = struct.unpack(">I", data[at : at + 4])
        kind = data[at + 4 : at + 8]
        assert at + 12 + n <= len(data), "a chunk's data runs past the end"
        body = data[at + 8 : at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n : at + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, f"CRC of the {kind!r} chunk at {at}"
        out.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return out


def inflate_raw(deflate: bytes) -> bytes:
    """A raw deflate stream (the segments of ``deflate`` / ``model_deflate``) back into its bytes; the stream must end exactly."""
    d = zlib.decompressobj(-15)
    out = d.decompress(deflate)
    assert d.eof and not d.unused_data, "the deflate stream does not end with its last block"
    return out


def unfilter(stream: np.ndarray, width: int, height: int, channels: int) -> tuple:
    """(bytes [height, width * channels], filter bytes [height]) of a filtered stream."""
    rows = stream.reshape(height, 1 + width * channels)
    out = np.zeros((height, width * channels), np.int32)
    zero = np.zeros(width * channels, np.int32)
    for y in range(height):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        up = out[y - 1] if y else zero
        assert f <= 4, f"filter byte {f} in row {y}"
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = (line + up) & 255
        elif f == 1:
            px = line.reshape(width, channels)
            out[y] = (np.cumsum(px, axis=0) & 255).reshape(-1)
        else:
            cur = out[y]
            for i in range(width * channels):
                a = cur[i - channels] if i >= channels else 0
                b = up[i]
                c = up[i - channels] if i >= channels else 0
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (line[i] + pred) & 255
    return out.astype(np.uint8), rows[:, 0].copy()


def read(data: bytes) -> dict:
    """A file of this encoder's kind: ``pixels`` [H, W, planes], ``alpha`` [H, W] or None, ``filters`` [H], ``colour_type``,
    ``idat`` (the payloads of the IDAT chunks), ``filtered`` (the inflated stream)."""
    assert data[:8] == SIGNATURE
    ch = chunks(data)
    assert ch[0][0] == b"IHDR" and len(ch[0][1]) == 13 and ch[-1] == (b"IEND", b"")
    assert all(k == b"IDAT" for k, _ in ch[1:-1]), "no ancillary chunk"
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in CHANNELS
    idat = [b for _, b in ch[1:-1]]
    d = zlib.decompressobj()
    stream = d.decompress(b"".join(idat))
    assert d.eof and not d.unused_data, "the zlib stream does not end with its Adler-32"
    c = CHANNELS[ctype]
    assert len(stream) == h * (1 + w * c)
    raw, filters = unfilter(np.frombuffer(stream, np.uint8), w, h, c)
    raw = raw.reshape(h, w, c)
    alpha = raw[:, :, -1].copy() if ctype in (4, 6) else None
    return {"pixels": raw[:, :, : c - (alpha is not None)].copy(), "alpha": alpha, "filters": filters, "colour_type": ctype, "idat": idat,
            "filtered": np.frombuffer(stream, np.uint8).reshape(h, -1)}


def frame(stream: bytes, width: int, height: int, colour_type: int) -> bytes:
    """PNG framing around a complete zlib stream: the yardstick's file."""
    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, colour_type, 0, 0, 0)) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")
