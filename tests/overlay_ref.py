"""An independent model of the overlay layer's integer rules, written from the text of include/meteor_demod_amd_overlay.h and
sharing nothing with csrc/overlay_host.cpp: the pieces of a polyline in Python integers (``math.isqrt``, ``//``), and coverage and
blend pixel by pixel.  Every piece is made, none is culled by the header's reach; a piece is evaluated on the pixels of a window of
its own around it (2 (w + 130) units on every side, more than any cap's corner), in numpy int64, whose ``>>`` and ``//`` are floors
and which the products stay far inside there."""
from __future__ import annotations

import math

import numpy as np

TOP = 1 << 30
PIECE_TOP = 16384


def cut(xs, ys, style):
    """The pieces (ax, ay, bx, by, tx, ty, L, style) of the polyline of integer vertices."""
    out = []
    for k in range(len(xs) - 1):
        ax, ay, bx, by = int(xs[k]), int(ys[k]), int(xs[k + 1]), int(ys[k + 1])
        if max(abs(ax), abs(ay), abs(bx), abs(by)) > TOP:
            continue
        dx, dy = bx - ax, by - ay
        k_pieces = max(1, -(-max(abs(dx), abs(dy)) // PIECE_TOP))
        vx = [ax + (2 * m * dx + k_pieces) // (2 * k_pieces) for m in range(k_pieces + 1)]
        vy = [ay + (2 * m * dy + k_pieces) // (2 * k_pieces) for m in range(k_pieces + 1)]
        for m in range(k_pieces):
            ex, ey = vx[m + 1] - vx[m], vy[m + 1] - vy[m]
            if ex == 0 and ey == 0:
                continue
            l16 = math.isqrt(256 * (ex * ex + ey * ey))
            out.append((vx[m], vy[m], vx[m + 1], vy[m + 1], (524288 * ex + l16) // (2 * l16), (524288 * ey + l16) // (2 * l16), (l16 + 8) >> 4, style))
    return out


def draw(pieces, styles, pixels, valid=None):
    """``styles``: a list of (half_width, opacity, colour, inside_only); ``pixels`` uint8 [H, W] or [H, W, 3].  (picture, mask)."""
    px = np.array(pixels, dtype=np.int64)
    h, w = px.shape[:2]
    planes = 1 if px.ndim == 2 else 3
    px = px.reshape(h, w, planes)
    top = np.zeros((len(styles), h, w), dtype=np.int64)
    for ax, ay, bx, by, tx, ty, length, s in pieces:
        half = styles[s][0]
        room = 2 * (half + 130)
        j0, j1 = max(0, -(-(min(ax, bx) - room) // 256)), min(w - 1, (max(ax, bx) + room) // 256)
        i0, i1 = max(0, -(-(min(ay, by) - room) // 256)), min(h - 1, (max(ay, by) + room) // 256)
        if j0 > j1 or i0 > i1:
            continue
        dx = 256 * np.arange(j0, j1 + 1, dtype=np.int64)[None, :] - ax
        dy = 256 * np.arange(i0, i1 + 1, dtype=np.int64)[:, None] - ay
        along = (tx * dx + ty * dy) >> 14
        perp = np.abs(tx * dy - ty * dx) >> 14
        d = np.maximum(np.maximum(perp, -along), np.maximum(along - length, 0))
        a = np.clip(half + 128 - d, 0, 256)
        top[s, i0:i1 + 1, j0:j1 + 1] = np.maximum(top[s, i0:i1 + 1, j0:j1 + 1], a)
    mask = np.zeros((h, w), dtype=np.uint8)
    for s, (half, opacity, colour, inside_only) in enumerate(styles):
        a = top[s]
        if inside_only:
            a = np.where(np.asarray(valid).reshape(h, w) != 0, a, 0)
        mask |= ((a > 0).astype(np.uint8) << s).astype(np.uint8)
        o = (a * opacity + 128) >> 8
        for p in range(planes):
            px[:, :, p] = (px[:, :, p] * (256 - o) + colour[p] * o + 128) >> 8
    out = px.astype(np.uint8)
    return (out[:, :, 0] if np.asarray(pixels).ndim == 2 else out), mask
