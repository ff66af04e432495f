"""The overlay layer: include/meteor_demod_amd_overlay.h over ctypes.

Lines on a latitude / longitude picture: ``read_vectors`` reads a shapefile's main file or a text file of ``lon lat`` lines,
``graticule`` makes meridians and parallels, ``project`` brings polylines to fixed point on a picture's grid, ``pieces`` cuts them,
``bins`` sorts the pieces into tiles, ``draw_pieces`` runs the kernel on device tensors, ``draw`` chains everything (numpy arrays go
through ``mdemod_overlay_draw_host``, in bands) and ``draw_map`` takes what ``map.image_to_map``, ``map.compose``,
``mosaic.compose`` and ``mosaic.images_to_mosaic`` return.  ``model_*`` is the host model of csrc/overlay_host.cpp, the kernel's
specification.  This module keeps its own binding tables, as every layer's does; ``_capi.bind`` applies them.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import check, take_bytes

MAX_STYLES = 4
TILE = 32


class MdemodOverlayGeo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("sx", C.c_uint32), ("reserved", C.c_uint32), ("sy", C.c_double), ("lat_top", C.c_double),
                ("lon_left", C.c_double)]


class MdemodOverlayVectors(C.Structure):
    _fields_ = [("lon", C.c_void_p), ("lat", C.c_void_p), ("first", C.c_void_p), ("n_lines", C.c_uint32), ("n_points", C.c_uint32), ("skipped", C.c_uint32),
                ("reserved", C.c_uint32)]


class MdemodOverlayPoints(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("first", C.c_void_p), ("n_lines", C.c_uint32), ("n_points", C.c_uint32)]


class MdemodOverlayPieces(C.Structure):
    _fields_ = [("piece", C.c_void_p), ("n", C.c_uint64), ("room", C.c_uint64)]


class MdemodOverlayStyle(C.Structure):
    _fields_ = [("half_width", C.c_uint32), ("opacity", C.c_uint32), ("colour", C.c_uint8 * 3), ("inside_only", C.c_uint8)]


class MdemodOverlayBins(C.Structure):
    _fields_ = [("tile_first", C.c_void_p), ("items", C.c_void_p), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("n_items", C.c_uint64)]


class MdemodOverlayLayer(C.Structure):
    _fields_ = [("vectors", C.POINTER(MdemodOverlayVectors)), ("style", C.c_uint32), ("reserved", C.c_uint32)]


class MdemodOverlayReport(C.Structure):
    _fields_ = [("pieces", C.c_uint64 * MAX_STYLES), ("pixels", C.c_uint64 * MAX_STYLES), ("tiles", C.c_uint64), ("items", C.c_uint64)]


PIECE = np.dtype([("ax", "<i4"), ("ay", "<i4"), ("tx", "<i4"), ("ty", "<i4"), ("L", "<i4"), ("style", "<i4"), ("zero", "<i4", (2,))])

_P = C.POINTER
_DRAW = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _P(MdemodOverlayStyle), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
         C.c_void_p]
_HOST = [_P(MdemodOverlayGeo), _P(MdemodOverlayLayer), C.c_uint32, _P(MdemodOverlayStyle), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
         _P(MdemodOverlayReport)]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_overlay.h
SIGNATURES = {
    "mdemod_overlay_read": (C.c_int, [C.c_char_p, _P(MdemodOverlayVectors)]),
    "mdemod_overlay_graticule": (C.c_int, [_P(MdemodOverlayGeo), C.c_double, _P(MdemodOverlayVectors)]),
    "mdemod_overlay_vectors_free": (None, [_P(MdemodOverlayVectors)]),
    "mdemod_overlay_project": (C.c_int, [_P(MdemodOverlayGeo), _P(MdemodOverlayVectors), _P(MdemodOverlayPoints)]),
    "mdemod_overlay_points_free": (None, [_P(MdemodOverlayPoints)]),
    "mdemod_overlay_cut": (C.c_int, [_P(MdemodOverlayPoints), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P(MdemodOverlayPieces)]),
    "mdemod_overlay_pieces_free": (None, [_P(MdemodOverlayPieces)]),
    "mdemod_overlay_bin": (C.c_int, [C.c_void_p, C.c_uint64, _P(MdemodOverlayStyle), C.c_uint32, C.c_uint32, C.c_uint32, _P(MdemodOverlayBins)]),
    "mdemod_overlay_bins_free": (None, [_P(MdemodOverlayBins)]),
    "mdemod_overlay_draw_device": (C.c_int, _DRAW + [C.c_int, C.c_void_p]),
    "mdemod_overlay_draw_host": (C.c_int, _HOST + [C.c_int]),
}
# the host model (csrc/overlay_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_overlay_model_draw": (C.c_int, [C.c_void_p, C.c_uint64, _P(MdemodOverlayStyle), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "mdemod_overlay_model_tiles": (C.c_int, _DRAW),
    "mdemod_overlay_model_host": (C.c_int, _HOST),
}


@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


# ------------------------------------------------------------------------------------------------------------------ values
@dataclass
class Geo:
    """A picture's grid: pixel (i, j) has its centre at ``lat_top - (i + 0.5) / sy`` and ``lon_left + (j + 0.5) / sx``."""
    width: int
    height: int
    sx: int
    sy: float
    lat_top: float
    lon_left: float


def geo_of(m) -> Geo:
    """The grid of a ``Geo``, a ``map.Map``, a ``mosaic.Mosaic`` or a grid of either layer."""
    return Geo(int(m.width), int(m.height), int(m.sx), float(m.sy), float(m.lat_top), float(m.lon_left))


def _geo(g) -> MdemodOverlayGeo:
    g = geo_of(g)
    return MdemodOverlayGeo(g.width, g.height, g.sx, 0, g.sy, g.lat_top, g.lon_left)


@dataclass
class Vectors:
    """Polylines in degrees: line l is ``lon[first[l]: first[l + 1]]``, ``lat[...]``; ``skipped`` counts a shapefile's records
    without a line."""
    lon: np.ndarray
    lat: np.ndarray
    first: np.ndarray
    skipped: int = 0

    @property
    def n_lines(self) -> int:
        return len(self.first) - 1

    def lines(self):
        return [(self.lon[a:b], self.lat[a:b]) for a, b in zip(self.first[:-1], self.first[1:])]


def vectors(lines) -> Vectors:
    """``lines``: a list of (lon array, lat array)."""
    lon = [np.asarray(a, dtype=np.float64).reshape(-1) for a, _ in lines]
    lat = [np.asarray(b, dtype=np.float64).reshape(-1) for _, b in lines]
    first = np.concatenate([[0], np.cumsum([len(a) for a in lon])]).astype(np.uint32)
    return Vectors(np.concatenate(lon) if lon else np.zeros(0), np.concatenate(lat) if lat else np.zeros(0), first)


def _c_vectors(v: Vectors):
    lon, lat = np.ascontiguousarray(v.lon, dtype=np.float64), np.ascontiguousarray(v.lat, dtype=np.float64)
    first = np.ascontiguousarray(v.first, dtype=np.uint32)
    if lon.shape != lat.shape or first.size < 1 or int(first[-1]) > lon.size:
        raise ValueError("the vectors' arrays do not fit each other")
    c = MdemodOverlayVectors(lon.ctypes.data, lat.ctypes.data, first.ctypes.data, first.size - 1, lon.size, int(v.skipped), 0)
    return c, (lon, lat, first)


def _take_vectors(c: MdemodOverlayVectors) -> Vectors:
    try:
        return Vectors(take_bytes(c.lon, c.n_points, np.float64), take_bytes(c.lat, c.n_points, np.float64), take_bytes(c.first, c.n_lines + 1, np.uint32), int(c.skipped))
    finally:
        lib().mdemod_overlay_vectors_free(C.byref(c))


def read_vectors(path) -> Vectors:
    """A shapefile's main file (.shp) or a text file of ``lon lat`` lines; a refusal is a ``MdemodError`` with the library's text."""
    c = MdemodOverlayVectors()
    check(lib().mdemod_overlay_read(os.fsencode(path), C.byref(c)), "mdemod_overlay_read")
    return _take_vectors(c)


def graticule(geo, step=0) -> Vectors:
    """The meridians and parallels at multiples of ``step`` degrees (0 or "auto": chosen from the scale) that cross the picture."""
    c = MdemodOverlayVectors()
    g = _geo(geo)
    check(lib().mdemod_overlay_graticule(C.byref(g), 0.0 if step == "auto" else float(step), C.byref(c)), "mdemod_overlay_graticule")
    return _take_vectors(c)


@dataclass
class Points:
    """Polylines in fixed point (1/256 pixel; pixel centres at multiples of 256)."""
    x: np.ndarray
    y: np.ndarray
    first: np.ndarray


def project(geo, v: Vectors) -> Points:
    c, keep = _c_vectors(v)
    g, p = _geo(geo), MdemodOverlayPoints()
    check(lib().mdemod_overlay_project(C.byref(g), C.byref(c), C.byref(p)), "mdemod_overlay_project")
    try:
        return Points(take_bytes(p.x, p.n_points, np.int32), take_bytes(p.y, p.n_points, np.int32), take_bytes(p.first, p.n_lines + 1, np.uint32))
    finally:
        lib().mdemod_overlay_points_free(C.byref(p))


def pieces(points: Points, style: int, half_width: int, width: int, height: int) -> np.ndarray:
    """The pieces (``PIECE`` records) of ``points`` that can reach a picture of width x height."""
    x, y = np.ascontiguousarray(points.x, dtype=np.int32), np.ascontiguousarray(points.y, dtype=np.int32)
    first = np.ascontiguousarray(points.first, dtype=np.uint32)
    if x.shape != y.shape or first.size < 1 or int(first[-1]) > x.size:
        raise ValueError("the points' arrays do not fit each other")
    c = MdemodOverlayPoints(x.ctypes.data, y.ctypes.data, first.ctypes.data, first.size - 1, x.size)
    out = MdemodOverlayPieces()
    try:
        check(lib().mdemod_overlay_cut(C.byref(c), int(style), int(half_width), int(width), int(height), C.byref(out)), "mdemod_overlay_cut")
        return take_bytes(out.piece, out.n, PIECE)
    finally:
        lib().mdemod_overlay_pieces_free(C.byref(out))


@dataclass
class Style:
    """``half_width`` in 1/256 pixel (128: a line of one pixel), ``opacity`` 0 .. 256."""
    half_width: int = 128
    opacity: int = 256
    colour: tuple = (255, 255, 0)
    inside_only: bool = False


def default_styles(colour=(255, 255, 0), width: float = 1.0) -> list:
    """Style 0 for coastlines (yellow, one pixel, opaque) and style 1 for the graticule (grey, one pixel, opacity 160): what the
    command-line program draws with."""
    return [Style(int(round(128 * width)), 256, tuple(colour), False), Style(128, 160, (128, 128, 128), False)]


def _styles(styles):
    arr = (MdemodOverlayStyle * max(len(styles), 1))()
    for k, s in enumerate(styles):
        arr[k].half_width, arr[k].opacity, arr[k].inside_only = int(s.half_width), int(s.opacity), int(bool(s.inside_only))
        for p in range(3):
            arr[k].colour[p] = int(s.colour[p])
    return arr


def layer_pieces(geo, layers, styles) -> np.ndarray:
    """The pieces of ``layers``, a list of (``Vectors``, style index), in the layers' order."""
    g = geo_of(geo)
    parts = [pieces(project(g, v), s, styles[s].half_width, g.width, g.height) for v, s in layers]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=PIECE)


def bins(pcs: np.ndarray, styles, width: int, height: int):
    """(tile_first, items) of the pieces: tiles of 32 x 32 pixels, row-major."""
    pcs = np.ascontiguousarray(pcs, dtype=PIECE)
    b = MdemodOverlayBins()
    check(lib().mdemod_overlay_bin(pcs.ctypes.data if pcs.size else None, pcs.size, _styles(styles), len(styles), int(width), int(height), C.byref(b)), "mdemod_overlay_bin")
    try:
        return take_bytes(b.tile_first, b.tiles_x * b.tiles_y + 1, np.uint32), take_bytes(b.items, b.n_items, np.uint32)
    finally:
        lib().mdemod_overlay_bins_free(C.byref(b))


def _planes(shape) -> int:
    if len(shape) == 2:
        return 1
    if len(shape) == 3 and shape[2] in (1, 3):
        return int(shape[2])
    raise ValueError(f"a picture is uint8 [H, W] or [H, W, 3], got {tuple(shape)}")


# ------------------------------------------------------------------------------------------------------------------ device
def draw_pieces(pixels, pcs, tile_first, items, styles, valid=None, mask: bool = False):
    """The kernel on a uint8 device tensor [H, W] or [H, W, 3], in place: ``pcs``, ``tile_first``, ``items`` as ``pieces`` and
    ``bins`` make them (numpy arrays are copied to the tensor's device).  With ``mask`` the uint8 [H, W] mask is returned.  On the
    current stream."""
    import torch
    if pixels.dtype != torch.uint8 or not pixels.is_contiguous():
        raise ValueError("the picture must be a contiguous uint8 tensor")
    planes = _planes(pixels.shape)
    h, w = int(pixels.shape[0]), int(pixels.shape[1])
    dev = pixels.device
    d = dev.index or 0

    def up(a, dtype):
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, dtype=dtype)
            return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)
        return a.contiguous()
    d_pcs, d_first, d_items = up(pcs, PIECE), up(tile_first, np.uint32), up(items, np.uint32)
    n_pieces, n_items = d_pcs.numel() * d_pcs.element_size() // PIECE.itemsize, d_items.numel() * d_items.element_size() // 4
    if valid is not None and (valid.dtype != torch.uint8 or tuple(valid.shape) != (h, w) or not valid.is_contiguous()):
        raise ValueError(f"valid must be a contiguous uint8 tensor [{h}, {w}]")
    out_mask = torch.empty((h, w), dtype=torch.uint8, device=dev) if mask else None
    check(lib().mdemod_overlay_draw_device(C.c_void_p(d_pcs.data_ptr()), n_pieces, C.c_void_p(d_first.data_ptr()), C.c_void_p(d_items.data_ptr()), n_items,
                                           _styles(styles), len(styles), w, h, planes, C.c_void_p(pixels.data_ptr()),
                                           C.c_void_p(valid.data_ptr()) if valid is not None else None, C.c_void_p(out_mask.data_ptr()) if mask else None, d,
                                           C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "mdemod_overlay_draw_device")
    return out_mask


@dataclass
class Report:
    """Per style the pieces kept and the pixels drawn; the tiles with an item; the items of all tiles."""
    pieces: list
    pixels: list
    tiles: int
    items: int


def _host(entry, name, pixels, geo, layers, styles, valid, mask, piece_lines, tail):
    g = geo_of(geo)
    px = np.array(pixels, dtype=np.uint8, order="C")                              # (a copy: the caller's picture stays)
    planes = _planes(px.shape)
    if px.shape[:2] != (g.height, g.width):
        raise ValueError(f"the picture is {px.shape[:2]}, the grid {g.height} x {g.width}")
    val = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    if val is not None and val.shape != (g.height, g.width):
        raise ValueError(f"valid must be uint8 [{g.height}, {g.width}]")
    msk = np.zeros((g.height, g.width), dtype=np.uint8)
    arr, keep = (MdemodOverlayLayer * max(len(layers), 1))(), []
    for k, (v, s) in enumerate(layers):
        c, held = _c_vectors(v)
        keep += [c, held]
        arr[k].vectors, arr[k].style = C.pointer(c), int(s)
    rep, cg = MdemodOverlayReport(), _geo(g)
    check(entry(C.byref(cg), arr, len(layers), _styles(styles), len(styles), planes, px.ctypes.data, val.ctypes.data if val is not None else None, msk.ctypes.data,
                int(piece_lines), C.byref(rep), *tail), name)
    n = len(styles)
    report = Report([int(rep.pieces[s]) for s in range(n)], [int(rep.pixels[s]) for s in range(n)], int(rep.tiles), int(rep.items))
    return px, msk, report


def draw_host(pixels, geo, layers, styles, valid=None, piece_lines: int = 0, device: int = 0):
    """``mdemod_overlay_draw_host`` on numpy arrays: (a drawn copy of the picture, the mask, the ``Report``)."""
    return _host(lib().mdemod_overlay_draw_host, "mdemod_overlay_draw_host", pixels, geo, layers, styles, valid, True, piece_lines, (int(device),))


def draw(pixels, geo, layers, styles, valid=None, mask: bool = False, piece_lines: int = 0, device: int = 0):
    """``layers``, a list of (``Vectors``, style index), drawn with ``styles`` (a list of ``Style``) onto a copy of ``pixels`` on the
    grid ``geo``: a uint8 device tensor (projected, cut and binned on the host, drawn by one launch on the tensor's device) or a numpy
    array (``draw_host``).  With ``mask`` the result is (picture, mask)."""
    if isinstance(pixels, np.ndarray):
        out, msk, _ = draw_host(pixels, geo, layers, styles, valid, piece_lines, device)
        return (out, msk) if mask else out
    g = geo_of(geo)
    pcs = layer_pieces(g, layers, styles)
    tile_first, items = bins(pcs, styles, g.width, g.height)
    out = pixels.contiguous().clone()
    msk = draw_pieces(out, pcs, tile_first, items, styles, valid=None if valid is None else valid.contiguous(), mask=mask)
    return (out, msk) if mask else out


def draw_map(m, layers, styles, device: int = 0, piece_lines: int = 0):
    """What ``map.image_to_map``, ``map.compose``, ``mosaic.compose`` or ``mosaic.images_to_mosaic`` returned with ``layers`` drawn
    on it: (picture, ``Report``); ``m.valid`` serves the styles that are inside_only."""
    out, _, report = draw_host(m.pixels, m, layers, styles, m.valid, piece_lines, device)
    return out, report


# ------------------------------------------------------------------------------------------------------------- the host model
def model_draw(pixels, geo, layers, styles, valid=None, mask: bool = False, piece_lines: int = 0):
    """``draw`` on numpy arrays by the host model (``mdemod_overlay_model_host``; no device)."""
    out, msk, _ = _host(lib().mdemod_overlay_model_host, "mdemod_overlay_model_host", pixels, geo, layers, styles, valid, True, piece_lines, ())
    return (out, msk) if mask else out


def _model_args(pixels, valid):
    px = np.array(pixels, dtype=np.uint8, order="C")
    planes = _planes(px.shape)
    h, w = px.shape[:2]
    val = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8).reshape(h, w)
    return px, planes, h, w, val, np.zeros((h, w), dtype=np.uint8)


def model_pieces(pixels, pcs, styles, valid=None):
    """The rule over every piece, pixel by pixel, without bins: (picture, mask)."""
    px, planes, h, w, val, msk = _model_args(pixels, valid)
    pcs = np.ascontiguousarray(pcs, dtype=PIECE)
    check(lib().mdemod_overlay_model_draw(pcs.ctypes.data if pcs.size else None, pcs.size, _styles(styles), len(styles), w, h, planes, px.ctypes.data,
                                          val.ctypes.data if val is not None else None, msk.ctypes.data), "mdemod_overlay_model_draw")
    return px, msk


def model_tiles(pixels, pcs, tile_first, items, styles, valid=None):
    """The model of the kernel on the kernel's arguments: (picture, mask)."""
    px, planes, h, w, val, msk = _model_args(pixels, valid)
    pcs, tile_first, items = np.ascontiguousarray(pcs, dtype=PIECE), np.ascontiguousarray(tile_first, dtype=np.uint32), np.ascontiguousarray(items, dtype=np.uint32)
    check(lib().mdemod_overlay_model_tiles(pcs.ctypes.data if pcs.size else None, pcs.size, tile_first.ctypes.data, items.ctypes.data if items.size else None, items.size,
                                           _styles(styles), len(styles), w, h, planes, px.ctypes.data, val.ctypes.data if val is not None else None, msk.ctypes.data),
          "mdemod_overlay_model_tiles")
    return px, msk
