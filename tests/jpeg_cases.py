"""What the CPU and the GPU tests of the JPEG encoder share: the test pictures, the crafted coefficient arrays, the float64 reference of
the coefficients, and small helpers around the host model (meteor_demod_amd.jpeg.model_*) and the test decoder (jpeg_ref.py)."""
from __future__ import annotations

import functools

import numpy as np

import jpeg_ref as R

SIZES = ((1, 1), (8, 8), (9, 9), (17, 23), (1568, 16), (2784, 8))               # width x height
QUALITIES = (1, 50, 90, 100)
INTERVALS = (1, 32, 64)


def picture(width: int, height: int, planes: int, seed: int = 0) -> np.ndarray:
    """A seeded picture with smooth ground, edges and a little noise: uint8 [H, W] or [H, W, 3]."""
    rng = np.random.default_rng(1000 * width + height + seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = 128 + 70 * np.sin(xx / 7.0) * np.cos(yy / 11.0) + 40 * np.sin((xx + 2 * yy) / 23.0) + 50 * ((xx // 13 + yy // 5) % 2)
    if planes == 1:
        return np.clip(base + rng.normal(0, 6, (height, width)), 0, 255).astype(np.uint8)
    rgb = np.stack([base, 0.8 * base + 30, 255 - base], axis=2) + rng.normal(0, 6, (height, width, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


@functools.cache
def psnr_pictures() -> dict:
    """The pictures of the coefficient and PSNR tests: smooth, noise and hard edges, at 136 x 96 and 83 x 61, colour."""
    rng = np.random.default_rng(5)
    out = {}
    for name, (h, w) in (("a", (96, 136)), ("b", (61, 83))):
        yy, xx = np.mgrid[0:h, 0:w]
        out["smooth_" + name] = picture(w, h, 3, 9)
        out["noise_" + name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        e = ((xx // 9 + yy // 7) % 2) * 200 + 20
        out["edges_" + name] = np.stack([e, 255 - e, e // 2 + rng.integers(0, 8, (h, w))], axis=2).astype(np.uint8)
    return out


def psnr(a, b) -> float:
    return float(10 * np.log10(255.0 ** 2 / max(((np.asarray(a, dtype=float) - np.asarray(b, dtype=float)) ** 2).mean(), 1e-12)))


def ycc(p: np.ndarray) -> np.ndarray:
    """The header's colour transform, in int64."""
    p = p.astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16], axis=-1)


def float_levels(pic: np.ndarray, q: np.ndarray):
    """(levels, quotients): round-half-away(float64 DCT / Q) with the header's clamp, and DCT / Q itself, [blocks, 64] in zig-zag
    order, the blocks of an MCU adjacent; q[2][64] as ``model_tables`` gives it."""
    planes = 1 if pic.ndim == 2 else 3
    s = (pic[..., None].astype(np.int64) if planes == 1 else ycc(pic)) - 128
    h, w = s.shape[:2]
    my, mx = (h + 7) // 8, (w + 7) // 8
    s = np.pad(s, ((0, my * 8 - h), (0, mx * 8 - w), (0, 0)), mode="edge").astype(float)
    c = R.dct_matrix()
    blocks = s.reshape(my, 8, mx, 8, planes).transpose(0, 2, 4, 1, 3).reshape(-1, 8, 8)
    F = np.einsum("ux,nxy,vy->nuv", c, blocks, c).reshape(my * mx, planes, 64)
    x = F / np.stack([q[0]] + [q[1]] * (planes - 1)).astype(float)[None]
    lv = np.sign(x) * np.floor(np.abs(x) + 0.5)
    lv[:, :, 0] = np.clip(lv[:, :, 0], -1024, 1023)
    lv[:, :, 1:] = np.clip(lv[:, :, 1:], -1023, 1023)
    return lv[:, :, R.ZIGZAG].reshape(-1, 64).astype(np.int64), x[:, :, R.ZIGZAG].reshape(-1, 64)


def clamped(coef: np.ndarray) -> np.ndarray:
    """What the entropy coder codes of any int16 coefficients."""
    out = np.clip(coef.astype(np.int32), -1023, 1023)
    out[:, 0] = np.clip(coef[:, 0].astype(np.int32), -1024, 1023)
    return out


DC_DIFFS = [s * d for k in range(11) for d in sorted({(1 << k) - 1, 1 << k} - {0}) for s in (1, -1)] + [2047, -2047]


@functools.cache
def crafted() -> np.ndarray:
    """int16 [105, 64], zig-zag order.  Zero runs of 15, 16, 17, 32 and 62 (the last with a non-zero coefficient 63: no EOB); all-zero
    blocks; pairs of blocks whose DC difference is every category edge +-(2^k - 1), +-2^k and +-2047 (the pairs stand at even
    places, so that an even restart interval keeps them together in a grey stream); blocks of the largest magnitude with alternating
    sign; a block of 63 x +1023, whose every coefficient is 16 + 10 bits with a run of 21 ones (an FF byte each) and which ends on an
    FF; values far outside the range; dense random blocks."""
    rng = np.random.default_rng(77)
    blocks = []
    for k, run in enumerate((15, 16, 17, 32, 62)):
        b = np.zeros(64, np.int32)
        b[0], b[1 + run] = 5 * k - 9, (-1) ** k * (3 + 40 * k)
        if run < 40:
            b[1 + run + 1 + 16] = 1                                               # a second run of exactly 16 behind it
        blocks.append(b)
    blocks.append(np.zeros(64, np.int32))
    for d in DC_DIFFS:
        prev = -((abs(d) + 1) // 2) if d > 0 else (abs(d) + 1) // 2 - 1
        a, b = np.zeros(64, np.int32), np.zeros(64, np.int32)
        a[0], b[0] = prev, prev + d
        a[1 + (abs(d) % 63)] = d % 7 - 3
        blocks += [a, b]
    blocks.append(np.zeros(64, np.int32))
    sign = np.where(np.arange(64) % 2 == 0, 1, -1)
    blocks += [1023 * sign, -1023 * sign - (np.arange(64) == 0), np.full(64, 1023, np.int32), 32767 * sign, -32768 * sign.clip(0, 1) + 32767 * (-sign).clip(0, 1)]
    blocks.append(np.zeros(64, np.int32))
    for _ in range(3):
        blocks.append(rng.integers(-1023, 1024, 64))
    blocks.append(np.full(64, 1023, np.int32))                                    # (the last block: the stream ends on an FF)
    out = np.array(blocks).astype(np.int16)
    assert out.shape == (105, 64), out.shape
    return out


def crafted_for(planes: int) -> np.ndarray:
    return crafted()[: (len(crafted()) // planes) * planes]


def split_segments(data: bytes) -> list:
    """The intervals of bare segments (00 bytes still in them): split at the RSTm, which no stuffed stream can hold."""
    parts, cur, p = [], bytearray(), 0
    while p < len(data):
        if data[p] == 0xFF and p + 1 < len(data) and 0xD0 <= data[p + 1] <= 0xD7:
            parts.append(bytes(cur))
            cur = bytearray()
            p += 2
        else:
            cur.append(data[p])
            p += 1
    parts.append(bytes(cur))
    return parts


def dht_of(J) -> dict:
    """The encoder's four tables as jpeg_ref takes them."""
    _, bits, vals, _, _ = J.model_tables(50)
    return {(k & 1, k >> 1): (bits[k], vals[k][: int(bits[k].sum())]) for k in range(4)}
