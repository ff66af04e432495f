"""The map layer: include/meteor_demod_amd_map.h over ctypes.

``parse_tle`` reads a two-line element set, ``fit_time`` fits the line times to the packets' onboard stamps, ``geolocate`` is the
forward function (pixel to latitude / longitude), ``grid`` makes the latitude / longitude grid with its nodes, ``warp`` resamples
the slots through the nodes on the GPU (device tensors in and out); ``compose`` chains them for numpy arrays (through
``mdemod_map_compose_host``, in bands) and ``image_to_map`` takes what ``image.vcdu_to_image`` returns.  ``model_*`` is the host
model of csrc/map_host.cpp over csrc/warp_model.h, the kernel's specification.  This module keeps its own binding tables, as every
layer's does; ``_capi.bind`` applies them.
"""
from __future__ import annotations

import ctypes as C
import datetime
import functools
from dataclasses import dataclass

import numpy as np

from . import _capi, picture
from ._capi import check, take_bytes
from .picture import _SLOTS, _dev_slots, _host_slots, _select, composite_select

NODE_STEP = 16
NO_NODE = -(1 << 31)
DATE_AUTO = -(1 << 31)


class MdemodMapTle(C.Structure):
    _fields_ = [("norad", C.c_uint32), ("epoch_day", C.c_int32), ("epoch_sec", C.c_double), ("inclination_deg", C.c_double), ("raan_deg", C.c_double),
                ("eccentricity", C.c_double), ("argp_deg", C.c_double), ("mean_anomaly_deg", C.c_double), ("mean_motion", C.c_double)]


class MdemodMapOpts(C.Structure):
    _fields_ = [("scan_deg", C.c_double), ("px_per_deg", C.c_double), ("time_offset", C.c_double), ("row_period", C.c_double), ("side", C.c_int32),
                ("date", C.c_int32), ("stretch", C.c_uint32), ("clip_low", C.c_uint32), ("clip_high", C.c_uint32), ("piece_lines", C.c_uint32)]


class MdemodMapTiming(C.Structure):
    _fields_ = [("row_period", C.c_double), ("s0", C.c_double), ("date", C.c_int32), ("rows_fit", C.c_uint32), ("placed", C.c_uint32), ("lines", C.c_uint32)]


class MdemodMapNodes(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("sx", C.c_uint32), ("node_rows", C.c_uint32), ("node_cols", C.c_uint32), ("date", C.c_int32),
                ("sy", C.c_double), ("lat_top", C.c_double), ("lon_left", C.c_double), ("nodes", C.c_void_p)]


class MdemodMapResult(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("planes", C.c_uint32), ("sx", C.c_uint32), ("sy", C.c_double), ("lat_top", C.c_double),
                ("lon_left", C.c_double), ("timing", MdemodMapTiming), ("utc0", C.c_double), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3),
                ("valid_pixels", C.c_uint64), ("pixels", C.c_void_p), ("valid", C.c_void_p)]


_P = C.POINTER
_WARP = [_P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
_COMPOSE = [_P(MdemodMapOpts), _P(MdemodMapTle), _P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
            _P(MdemodMapResult)]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_map.h
SIGNATURES = {
    "mdemod_map_default_opts": (None, [_P(MdemodMapOpts)]),
    "mdemod_map_parse_tle": (C.c_int, [C.c_char_p, C.c_uint32, _P(MdemodMapTle)]),
    "mdemod_map_fit_time": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, _P(MdemodMapOpts), _P(MdemodMapTiming)]),
    "mdemod_map_date": (C.c_int, [_P(MdemodMapTle), _P(MdemodMapTiming), _P(MdemodMapOpts), _P(C.c_int32)]),
    "mdemod_map_geolocate": (C.c_int, [_P(MdemodMapTle), _P(MdemodMapTiming), _P(MdemodMapOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mdemod_map_grid": (C.c_int, [_P(MdemodMapTle), _P(MdemodMapTiming), _P(MdemodMapOpts), C.c_uint32, _P(MdemodMapNodes)]),
    "mdemod_map_grid_free": (None, [_P(MdemodMapNodes)]),
    "mdemod_map_warp_device": (C.c_int, _WARP + [C.c_int, C.c_void_p]),
    "mdemod_map_compose_host": (C.c_int, _COMPOSE + [C.c_int]),
    "mdemod_map_free": (None, [_P(MdemodMapResult)]),
}
# the host model (csrc/map_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_map_model_warp": (C.c_int, _WARP),
    "mdemod_map_model_host": (C.c_int, _COMPOSE),
}
PLACEMENT = np.dtype([("channel", "<i4"), ("row", "<u4"), ("cell", "<u4"), ("reserved", "<u4")])
STRIP_INFO = np.dtype([("mcus", "u1"), ("q", "u1"), ("mcun", "u1"), ("flags", "u1"), ("day", "<u2"), ("us", "<u2"), ("ms", "<u4"), ("bits_used", "<u4")])

@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed, and the picture layer's, whose histogram and tables this layer's callers
    use beside it (the same handle as ``_capi.lib()``)."""
    picture.lib()
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


_FLOATS = ("scan_deg", "px_per_deg", "time_offset", "row_period")


def _date(value) -> int:
    """A date option: None / "auto", days since 1970-01-01, a ``datetime.date`` or "yyyy-mm-dd"."""
    if value is None or value == "auto":
        return DATE_AUTO
    if isinstance(value, str):
        value = datetime.date.fromisoformat(value)
    if isinstance(value, datetime.date):
        return (value - datetime.date(1970, 1, 1)).days
    return int(value)


def make_opts(**opts) -> MdemodMapOpts:
    """``mdemod_map_default_opts`` with the given fields replaced (an unknown name is a TypeError)."""
    o = MdemodMapOpts()
    lib().mdemod_map_default_opts(C.byref(o))
    names = {f[0] for f in MdemodMapOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"map: no option {k!r} (there are: {', '.join(sorted(names))})")
        setattr(o, k, float(v) if k in _FLOATS else _date(v) if k == "date" else int(v))
    return o


def parse_tle(text, norad: int = 0) -> MdemodMapTle:
    """The first element set of ``text`` (str or bytes), or the one with the catalogue number ``norad``."""
    raw = text.encode("latin-1", "replace") if isinstance(text, str) else bytes(text)
    if b"\0" in raw:
        raw = raw[: raw.index(b"\0")]
    tle = MdemodMapTle()
    check(lib().mdemod_map_parse_tle(raw, int(norad), C.byref(tle)), "mdemod_map_parse_tle")
    return tle


def _tle(tle, norad=0) -> MdemodMapTle:
    return tle if isinstance(tle, MdemodMapTle) else parse_tle(tle, norad)


def _packets(place, sinfo):
    p = np.ascontiguousarray(place, dtype=PLACEMENT)
    s = np.ascontiguousarray(sinfo, dtype=STRIP_INFO)
    if p.shape != s.shape or p.ndim != 1:
        raise ValueError(f"placements {p.shape} and reports {s.shape} must be lists of the same length")
    return p, s


def fit_time(place, sinfo, **opts) -> MdemodMapTiming:
    """The line times from the placements and reports of the packets (structured arrays as ``image`` returns them)."""
    p, s = _packets(place, sinfo)
    o, t = make_opts(**opts), MdemodMapTiming()
    check(lib().mdemod_map_fit_time(p.ctypes.data if p.size else None, s.ctypes.data if s.size else None, p.size, C.byref(o), C.byref(t)), "mdemod_map_fit_time")
    return t


def resolve_date(tle, timing: MdemodMapTiming, **opts) -> int:
    """The date (days since 1970-01-01) the line times stand for: the timing's own, or for "auto" the one nearest the epoch."""
    o, d = make_opts(**opts), C.c_int32(0)
    check(lib().mdemod_map_date(C.byref(_tle(tle)), C.byref(timing), C.byref(o), C.byref(d)), "mdemod_map_date")
    return d.value


def geolocate(tle, timing: MdemodMapTiming, y, x, **opts):
    """Pixels (line ``y``, column ``x``; arrays of one shape) to (lat, lon) in degrees; NaN where the pixel does not see the Earth."""
    o = make_opts(**opts)
    ya, xa = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
    if ya.shape != xa.shape:
        raise ValueError("y and x differ in shape")
    lat, lon = np.empty(ya.shape), np.empty(ya.shape)
    check(lib().mdemod_map_geolocate(C.byref(_tle(tle)), C.byref(timing), C.byref(o), ya.ctypes.data, xa.ctypes.data, ya.size, lat.ctypes.data, lon.ctypes.data),
          "mdemod_map_geolocate")
    return lat, lon


@dataclass
class Grid:
    """``nodes`` int32 [node rows, node cols, 2] (X, Y in 1/256 source pixel, NO_NODE in both where there is none); pixel (i, j) has
    its centre at ``lat_top - (i + 0.5) / sy`` and ``lon_left + (j + 0.5) / sx``."""
    width: int
    height: int
    sx: int
    sy: float
    lat_top: float
    lon_left: float
    date: int
    nodes: np.ndarray

    def world_file(self) -> str:
        return world_file(self.sx, self.sy, self.lat_top, self.lon_left)


def world_file(sx, sy, lat_top, lon_left) -> str:
    """The six lines of the world file, with enough digits to read back the same doubles."""
    return "".join(f"{v!r}\n" for v in (1.0 / sx, 0.0, 0.0, -1.0 / sy, lon_left + 0.5 / sx, lat_top - 0.5 / sy))


def grid(tle, timing: MdemodMapTiming, lines: int, **opts) -> Grid:
    o, g = make_opts(**opts), MdemodMapNodes()
    check(lib().mdemod_map_grid(C.byref(_tle(tle)), C.byref(timing), C.byref(o), int(lines), C.byref(g)), "mdemod_map_grid")
    try:
        nodes = np.frombuffer(C.string_at(g.nodes, 8 * g.node_rows * g.node_cols), dtype=np.int32).reshape(g.node_rows, g.node_cols, 2).copy()
        return Grid(int(g.width), int(g.height), int(g.sx), float(g.sy), float(g.lat_top), float(g.lon_left), int(g.date), nodes)
    finally:
        lib().mdemod_map_grid_free(C.byref(g))


def _nodes_shape(width, height):
    return (-(-height // NODE_STEP) + 1, -(-width // NODE_STEP) + 1, 2)


def warp(images, filled, select, luts, nodes, width: int, height: int, valid: bool = False):
    """The slots ``select`` (1 or 3 of them; device tensors) through the tables ``luts`` (uint8 [planes, 256]) and ``nodes`` (int32
    [ceil(height / 16) + 1, ceil(width / 16) + 1, 2]) into a uint8 [height, width, planes] device tensor; with ``valid`` also the
    uint8 [height, width] one.  ``luts`` and ``nodes`` may be numpy arrays (copied to the device) or device tensors.  On the current
    stream."""
    import torch
    sel, planes = _select(select)
    chosen = [images[s] if s in select else None for s in range(3)]
    pi, pf, rows, dev, keep = _dev_slots(chosen, filled)
    d = dev.index or 0
    if isinstance(luts, np.ndarray):
        luts = torch.from_numpy(np.ascontiguousarray(luts, dtype=np.uint8)).to(dev)
    if isinstance(nodes, np.ndarray):
        nodes = torch.from_numpy(np.ascontiguousarray(nodes, dtype=np.int32)).to(dev)
    luts, nodes = luts.contiguous(), nodes.contiguous()
    if luts.dtype != torch.uint8 or luts.numel() != 256 * planes:
        raise ValueError(f"the tables must be uint8 [{planes}, 256]")
    if nodes.dtype != torch.int32 or tuple(nodes.shape) != _nodes_shape(width, height):
        raise ValueError(f"the nodes must be int32 {_nodes_shape(width, height)}, got {nodes.dtype} {tuple(nodes.shape)}")
    out = torch.empty((height, width, planes), dtype=torch.uint8, device=dev)
    val = torch.empty((height, width), dtype=torch.uint8, device=dev) if valid else None
    check(lib().mdemod_map_warp_device(C.byref(pi), C.byref(pf), rows, sel, planes, C.c_void_p(luts.data_ptr()), C.c_void_p(nodes.data_ptr()), int(width), int(height),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(val.data_ptr()) if valid else None, d,
                                       C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "mdemod_map_warp_device")
    return (out, val) if valid else out


@dataclass
class Map:
    """``pixels`` uint8 [H, W] (grey) or [H, W, 3]; ``valid`` uint8 [H, W], bit p: plane p had a filled tap; ``limits`` the (lo, hi)
    of each plane's stretch; ``select`` the slot of each plane; ``timing`` the fitted line times with the date that was used;
    ``utc0`` the UTC seconds of that date of line 0."""
    pixels: np.ndarray
    valid: np.ndarray
    limits: list
    select: tuple
    sx: int
    sy: float
    lat_top: float
    lon_left: float
    row_period: float
    rows_fit: int
    date: int
    utc0: float

    @property
    def width(self) -> int:
        return int(self.pixels.shape[1])

    @property
    def height(self) -> int:
        return int(self.pixels.shape[0])

    @property
    def valid_share(self) -> float:
        return float(np.count_nonzero(self.valid)) / self.valid.size if self.valid.size else 0.0

    def world_file(self) -> str:
        return world_file(self.sx, self.sy, self.lat_top, self.lon_left)

    def first_line_utc(self) -> datetime.datetime:
        return datetime.datetime(1970, 1, 1) + datetime.timedelta(days=self.date, seconds=self.utc0)


def _take(res: MdemodMapResult, select) -> Map:
    """A C result into arrays of our own; the C side's memory goes back."""
    try:
        w, h, planes = int(res.width), int(res.height), int(res.planes)
        px = take_bytes(res.pixels, h * w * planes).reshape((h, w, planes) if planes == 3 else (h, w))
        return Map(px, take_bytes(res.valid, h * w).reshape(h, w), [(int(res.lo[p]), int(res.hi[p])) for p in range(planes)], tuple(int(s) for s in select),
                   int(res.sx), float(res.sy), float(res.lat_top), float(res.lon_left), float(res.timing.row_period), int(res.timing.rows_fit),
                   int(res.timing.date), float(res.utc0))
    finally:
        lib().mdemod_map_free(C.byref(res))


def _compose(entry, name, tle, images, filled, place, sinfo, select, tail, norad, opts) -> Map:
    o = make_opts(**opts)
    sel, planes = _select(select)
    pi, pf, rows, keep = _host_slots(images, filled)
    p, s = _packets(place, sinfo)
    res = MdemodMapResult()
    check(entry(C.byref(o), C.byref(_tle(tle, norad)), C.byref(pi), C.byref(pf), rows, p.ctypes.data if p.size else None, s.ctypes.data if s.size else None,
                p.size, sel, planes, C.byref(res), *tail), name)
    return _take(res, select)


def compose(tle, images, filled, place, sinfo, select=(2, 1, 0), device: int = 0, norad: int = 0, **opts) -> Map:
    """Pictures and masks of the three slots (numpy arrays), the packets' placements and reports and a TLE (text or parsed) to the
    finished ``Map`` through ``mdemod_map_compose_host`` (in bands of ``piece_lines``; ``device`` says where)."""
    return _compose(lib().mdemod_map_compose_host, "mdemod_map_compose_host", tle, images, filled, place, sinfo, select, (int(device),), norad, opts)


def image_to_map(result, tle_text, composite="auto", device: int = 0, norad: int = 0, **opts) -> Map | None:
    """An ``image.Result`` and a TLE to a ``Map``: the slots are the result's channels in the order of its APIDs.  Mirrors
    ``picture.image_to_picture``."""
    apids = list(result.images)
    images, filled = [result.images[a] for a in apids], [result.filled[a] for a in apids]
    select = composite_select(composite, [f.any() for f in filled])
    if select is None:
        return None
    return compose(tle_text, images, filled, result.place, result.sinfo, select, device=device, norad=norad, **opts)


# ------------------------------------------------------------------------------------------------------------- the host model
def model_warp(images, filled, select, luts, nodes, width: int, height: int, valid: bool = False):
    """(uint8 [height, width, planes], and with ``valid`` uint8 [height, width]) of the host model."""
    sel, planes = _select(select)
    pi, pf, rows, keep = _host_slots(images, filled)
    t = np.ascontiguousarray(luts, dtype=np.uint8).reshape(planes, 256)
    n = np.ascontiguousarray(nodes, dtype=np.int32)
    if n.shape != _nodes_shape(width, height):
        raise ValueError(f"the nodes must be int32 {_nodes_shape(width, height)}, got {n.shape}")
    out = np.zeros((height, width, planes), dtype=np.uint8)
    val = np.zeros((height, width), dtype=np.uint8)
    check(lib().mdemod_map_model_warp(C.byref(pi), C.byref(pf), rows, sel, planes, t.ctypes.data, n.ctypes.data, int(width), int(height), out.ctypes.data,
                                      val.ctypes.data if valid else None), "mdemod_map_model_warp")
    return (out, val) if valid else out


def model_host(tle, images, filled, place, sinfo, select=(2, 1, 0), norad: int = 0, **opts) -> Map:
    """``mdemod_map_compose_host`` with the model in the kernel's place (no device): the time fit, the grid, the tables, the bands."""
    return _compose(lib().mdemod_map_model_host, "mdemod_map_model_host", tle, images, filled, place, sinfo, select, (), norad, opts)
