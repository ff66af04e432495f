"""The mosaic layer: include/meteor_demod_amd_mosaic.h over ctypes.

Several passes, each what ``map.compose`` takes for one map, blended onto one latitude / longitude grid.  ``grid`` makes the common
grid with every pass's nodes, ``blend`` blends device tensors through given nodes and tables on the GPU, ``compose`` chains
everything for numpy arrays (through ``mdemod_mosaic_compose_host``, in bands) and ``images_to_mosaic`` takes a list of what
``image.vcdu_to_image`` returns.  ``model_*`` is the host model of csrc/mosaic_host.cpp over csrc/warp_model.h, the kernel's
specification.  This module keeps its own binding tables, as every layer's does; ``_capi.bind`` applies them.
"""
from __future__ import annotations

import ctypes as C
import datetime
import functools
from dataclasses import dataclass, field

import numpy as np

from . import _capi, map as _map
from ._capi import check, take_bytes
from .map import _date, _nodes_shape, _packets, world_file
from .picture import _SLOTS, _dev_slots, _host_slots, _select, composite_select

MAX_PASSES = 8
FEATHER, BEST = 0, 1
BLENDS = {"feather": FEATHER, "best": BEST}
DATE_AUTO = -(1 << 31)
NO_NODE = -(1 << 31)


class MdemodMosaicOpts(C.Structure):
    _fields_ = [("scan_deg", C.c_double), ("px_per_deg", C.c_double), ("time_offset", C.c_double), ("row_period", C.c_double), ("side", C.c_int32),
                ("stretch", C.c_uint32), ("clip_low", C.c_uint32), ("clip_high", C.c_uint32), ("piece_lines", C.c_uint32), ("blend", C.c_uint32)]


class MdemodMosaicPass(C.Structure):
    _fields_ = [("tle_text", C.c_char_p), ("norad", C.c_uint32), ("date", C.c_int32), ("image", _SLOTS), ("filled", _SLOTS), ("rows", C.c_uint32),
                ("reserved", C.c_uint32), ("place", C.c_void_p), ("sinfo", C.c_void_p), ("n_desc", C.c_uint64)]


class MdemodMosaicTiming(C.Structure):
    _fields_ = [("row_period", C.c_double), ("s0", C.c_double), ("date", C.c_int32), ("rows_fit", C.c_uint32), ("placed", C.c_uint32), ("lines", C.c_uint32)]


class MdemodMosaicNodes(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("sx", C.c_uint32), ("node_rows", C.c_uint32), ("node_cols", C.c_uint32), ("n", C.c_uint32),
                ("sy", C.c_double), ("lat_top", C.c_double), ("lon_left", C.c_double), ("timing", MdemodMosaicTiming * MAX_PASSES),
                ("nodes", C.c_void_p * MAX_PASSES)]


class MdemodMosaicSource(C.Structure):
    _fields_ = [("image", _SLOTS), ("filled", _SLOTS), ("lut", C.c_void_p), ("nodes", C.c_void_p), ("rows", C.c_uint32), ("reserved", C.c_uint32)]


class MdemodMosaicResult(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("planes", C.c_uint32), ("sx", C.c_uint32), ("n", C.c_uint32), ("blend", C.c_uint32),
                ("sy", C.c_double), ("lat_top", C.c_double), ("lon_left", C.c_double), ("timing", MdemodMosaicTiming * MAX_PASSES),
                ("utc0", C.c_double * MAX_PASSES), ("lo", (C.c_uint32 * 3) * MAX_PASSES), ("hi", (C.c_uint32 * 3) * MAX_PASSES),
                ("covered", C.c_uint64 * MAX_PASSES), ("valid_pixels", C.c_uint64), ("overlap_pixels", C.c_uint64), ("pixels", C.c_void_p),
                ("valid", C.c_void_p), ("cover", C.c_void_p)]


_P = C.POINTER
_BLEND = [_P(MdemodMosaicSource), C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
_COMPOSE = [_P(MdemodMosaicOpts), _P(MdemodMosaicPass), C.c_uint32, C.c_void_p, C.c_uint32, _P(MdemodMosaicResult)]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_mosaic.h
SIGNATURES = {
    "mdemod_mosaic_default_opts": (None, [_P(MdemodMosaicOpts)]),
    "mdemod_mosaic_grid": (C.c_int, [_P(MdemodMosaicOpts), _P(MdemodMosaicPass), C.c_uint32, _P(MdemodMosaicNodes)]),
    "mdemod_mosaic_grid_free": (None, [_P(MdemodMosaicNodes)]),
    "mdemod_mosaic_blend_device": (C.c_int, _BLEND + [C.c_int, C.c_void_p]),
    "mdemod_mosaic_compose_host": (C.c_int, _COMPOSE + [C.c_int]),
    "mdemod_mosaic_free": (None, [_P(MdemodMosaicResult)]),
}
# the host model (csrc/mosaic_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_mosaic_model_blend": (C.c_int, _BLEND),
    "mdemod_mosaic_model_host": (C.c_int, _COMPOSE),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed, and those of the map and picture layers under it (the same handle as
    ``_capi.lib()``)."""
    _map.lib()
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


_FLOATS = ("scan_deg", "px_per_deg", "time_offset", "row_period")


def make_opts(**opts) -> MdemodMosaicOpts:
    """``mdemod_mosaic_default_opts`` with the given fields replaced (an unknown name is a TypeError); ``blend`` may be "feather" or
    "best"."""
    o = MdemodMosaicOpts()
    lib().mdemod_mosaic_default_opts(C.byref(o))
    names = {f[0] for f in MdemodMosaicOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"mosaic: no option {k!r} (there are: {', '.join(sorted(names))})")
        setattr(o, k, float(v) if k in _FLOATS else BLENDS[v] if k == "blend" and isinstance(v, str) else int(v))
    return o


@dataclass
class Pass:
    """One pass as the mosaic takes it: TLE text, pictures and masks of the three slots (numpy; a slot may be None), the packets'
    placements and reports; ``norad`` 0 is the text's first set, ``date`` as ``map.make_opts`` takes it."""
    tle_text: str
    images: list
    filled: list
    place: np.ndarray
    sinfo: np.ndarray
    norad: int = 0
    date: object = None


def _passes(passes):
    """The C array of the passes, and what must outlive the call."""
    arr, keep = (MdemodMosaicPass * max(len(passes), 1))(), []
    for k, p in enumerate(passes):
        raw = p.tle_text.encode("latin-1", "replace") if isinstance(p.tle_text, str) else bytes(p.tle_text)
        place, sinfo = _packets(p.place, p.sinfo)
        keep += [raw, place, sinfo]
        c = arr[k]
        c.tle_text, c.norad, c.date = raw.split(b"\0")[0], int(p.norad), _date(p.date)
        pi, pf, rows, held = _host_slots(p.images, p.filled)
        keep += held
        for s in range(3):
            c.image[s], c.filled[s] = pi[s], pf[s]
        c.rows = rows
        c.place, c.sinfo, c.n_desc = (place.ctypes.data if place.size else None), (sinfo.ctypes.data if sinfo.size else None), place.size
    return arr, keep


@dataclass
class PassRecord:
    """What the mosaic reports per pass: the fitted line times with the date that was used, ``utc0`` the UTC seconds of that date of
    line 0, ``limits`` the (lo, hi) of each plane's stretch, ``covered`` the pixels the pass counted in."""
    row_period: float
    s0: float
    rows_fit: int
    placed: int
    lines: int
    date: int
    utc0: float = 0.0
    limits: list = field(default_factory=list)
    covered: int = 0

    def first_line_utc(self) -> datetime.datetime:
        return datetime.datetime(1970, 1, 1) + datetime.timedelta(days=self.date, seconds=self.utc0)


def _record(t: MdemodMosaicTiming) -> PassRecord:
    return PassRecord(float(t.row_period), float(t.s0), int(t.rows_fit), int(t.placed), int(t.lines), int(t.date))


@dataclass
class Grid:
    """The common grid: ``nodes`` int32 [passes, node rows, node cols, 2]; pixel (i, j) has its centre at
    ``lat_top - (i + 0.5) / sy`` and ``lon_left + (j + 0.5) / sx``."""
    width: int
    height: int
    sx: int
    sy: float
    lat_top: float
    lon_left: float
    nodes: np.ndarray
    passes: list

    def world_file(self) -> str:
        return world_file(self.sx, self.sy, self.lat_top, self.lon_left)


def grid(passes, **opts) -> Grid:
    """The common grid of ``passes`` (a list of ``Pass``; one slot's picture is enough: it says how many strip rows the pass has) with
    every pass's nodes and resolved line times."""
    o, g = make_opts(**opts), MdemodMosaicNodes()
    arr, keep = _passes(passes)
    check(lib().mdemod_mosaic_grid(C.byref(o), arr, len(passes), C.byref(g)), "mdemod_mosaic_grid")
    try:
        count = 8 * g.node_rows * g.node_cols
        nodes = np.stack([np.frombuffer(C.string_at(g.nodes[k], count), dtype=np.int32).reshape(g.node_rows, g.node_cols, 2) for k in range(g.n)])
        return Grid(int(g.width), int(g.height), int(g.sx), float(g.sy), float(g.lat_top), float(g.lon_left), nodes, [_record(g.timing[k]) for k in range(g.n)])
    finally:
        lib().mdemod_mosaic_grid_free(C.byref(g))


def _blend_mode(blend) -> int:
    return BLENDS[blend] if isinstance(blend, str) else int(blend)


def blend(sources, select, width: int, height: int, blend="feather", valid: bool = False, cover: bool = False):
    """``sources``: a list of (images, filled, luts, nodes) per pass, device tensors as ``map.warp`` takes them (``luts`` and
    ``nodes`` may be numpy arrays), or None for an empty pass.  The slots ``select`` of every pass blended into a uint8
    [height, width, planes] device tensor; with ``valid`` / ``cover`` also those uint8 [height, width] tensors, in that order.  On the
    current stream."""
    import torch
    sel, planes = _select(select)
    arr, keep, dev = (MdemodMosaicSource * max(len(sources), 1))(), [], None
    for k, src in enumerate(sources):
        if src is None:
            continue
        images, filled, luts, nodes = src
        chosen = [images[s] if s in select else None for s in range(3)]
        pi, pf, rows, dev, held = _dev_slots(chosen, filled)
        if isinstance(luts, np.ndarray):
            luts = torch.from_numpy(np.ascontiguousarray(luts, dtype=np.uint8)).to(dev)
        if isinstance(nodes, np.ndarray):
            nodes = torch.from_numpy(np.ascontiguousarray(nodes, dtype=np.int32)).to(dev)
        luts, nodes = luts.contiguous(), nodes.contiguous()
        if luts.dtype != torch.uint8 or luts.numel() != 256 * planes:
            raise ValueError(f"the tables must be uint8 [{planes}, 256]")
        if nodes.dtype != torch.int32 or tuple(nodes.shape) != _nodes_shape(width, height):
            raise ValueError(f"the nodes must be int32 {_nodes_shape(width, height)}, got {nodes.dtype} {tuple(nodes.shape)}")
        keep += held + [luts, nodes]
        for s in range(3):
            arr[k].image[s], arr[k].filled[s] = pi[s], pf[s]
        arr[k].lut, arr[k].nodes, arr[k].rows = luts.data_ptr(), nodes.data_ptr(), rows
    if dev is None:
        raise ValueError("no pass given")
    d = dev.index or 0
    out = torch.empty((height, width, planes), dtype=torch.uint8, device=dev)
    val = torch.empty((height, width), dtype=torch.uint8, device=dev) if valid else None
    cov = torch.empty((height, width), dtype=torch.uint8, device=dev) if cover else None
    check(lib().mdemod_mosaic_blend_device(arr, len(sources), sel, planes, _blend_mode(blend), int(width), int(height), C.c_void_p(out.data_ptr()),
                                           C.c_void_p(val.data_ptr()) if valid else None, C.c_void_p(cov.data_ptr()) if cover else None, d,
                                           C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "mdemod_mosaic_blend_device")
    extra = [x for x in (val, cov) if x is not None]
    return (out, *extra) if extra else out


@dataclass
class Mosaic:
    """``pixels`` uint8 [H, W] (grey) or [H, W, 3]; ``valid`` uint8 [H, W], bit p: plane p had a counting pass; ``cover`` uint8
    [H, W], bit k: pass k counted; ``select`` the slot of each plane; ``passes`` one ``PassRecord`` per pass."""
    pixels: np.ndarray
    valid: np.ndarray
    cover: np.ndarray
    select: tuple
    sx: int
    sy: float
    lat_top: float
    lon_left: float
    blend: int
    passes: list
    valid_pixels: int
    overlap_pixels: int

    @property
    def width(self) -> int:
        return int(self.pixels.shape[1])

    @property
    def height(self) -> int:
        return int(self.pixels.shape[0])

    @property
    def valid_share(self) -> float:
        return float(self.valid_pixels) / self.valid.size if self.valid.size else 0.0

    @property
    def overlap_share(self) -> float:
        return float(self.overlap_pixels) / self.cover.size if self.cover.size else 0.0

    def world_file(self) -> str:
        return world_file(self.sx, self.sy, self.lat_top, self.lon_left)


def _take(res: MdemodMosaicResult, select) -> Mosaic:
    """A C result into arrays of our own; the C side's memory goes back."""
    try:
        w, h, planes, n = int(res.width), int(res.height), int(res.planes), int(res.n)
        px = take_bytes(res.pixels, h * w * planes).reshape((h, w, planes) if planes == 3 else (h, w))
        records = []
        for k in range(n):
            r = _record(res.timing[k])
            r.utc0, r.covered = float(res.utc0[k]), int(res.covered[k])
            r.limits = [(int(res.lo[k][p]), int(res.hi[k][p])) for p in range(planes)]
            records.append(r)
        return Mosaic(px, take_bytes(res.valid, h * w).reshape(h, w), take_bytes(res.cover, h * w).reshape(h, w),tuple(int(s) for s in select), int(res.sx), float(res.sy),
                      float(res.lat_top), float(res.lon_left), int(res.blend), records, int(res.valid_pixels), int(res.overlap_pixels))
    finally:
        lib().mdemod_mosaic_free(C.byref(res))


def _compose(entry, name, passes, select, tail, opts) -> Mosaic:
    o = make_opts(**opts)
    sel, planes = _select(select)
    arr, keep = _passes(passes)
    res = MdemodMosaicResult()
    check(entry(C.byref(o), arr, len(passes), sel, planes, C.byref(res), *tail), name)
    return _take(res, select)


def compose(passes, select=(2, 1, 0), device: int = 0, **opts) -> Mosaic:
    """A list of ``Pass`` (numpy arrays) to the finished ``Mosaic`` through ``mdemod_mosaic_compose_host`` (in bands of
    ``piece_lines``; ``device`` says where)."""
    return _compose(lib().mdemod_mosaic_compose_host, "mdemod_mosaic_compose_host", passes, select, (int(device),), opts)


def images_to_mosaic(results, tle_text, composite="auto", device: int = 0, norad: int = 0, date=None, **opts) -> Mosaic | None:
    """A list of ``image.Result`` (one per pass, all of the satellite of ``tle_text``) to a ``Mosaic``: the slots are the results'
    channels in the order of their APIDs; ``composite`` "auto" is resolved on the union of what the passes received."""
    passes, received = [], [False, False, False]
    for result in results:
        apids = list(result.images)
        images, filled = [result.images[a] for a in apids], [result.filled[a] for a in apids]
        received = [r or bool(f.any()) for r, f in zip(received, filled)]
        passes.append(Pass(tle_text, images, filled, result.place, result.sinfo, norad=norad, date=date))
    select = composite_select(composite, received)
    if select is None:
        return None
    return compose(passes, select, device=device, **opts)


# ------------------------------------------------------------------------------------------------------------- the host model
def model_blend(sources, select, width: int, height: int, blend="feather", valid: bool = False, cover: bool = False):
    """``blend`` on numpy arrays by the host model: ``sources`` a list of (images, filled, luts, nodes) or None."""
    sel, planes = _select(select)
    arr, keep = (MdemodMosaicSource * max(len(sources), 1))(), []
    for k, src in enumerate(sources):
        if src is None:
            continue
        images, filled, luts, nodes = src
        pi, pf, rows, held = _host_slots(images, filled)
        t = np.ascontiguousarray(luts, dtype=np.uint8).reshape(planes, 256)
        n = np.ascontiguousarray(nodes, dtype=np.int32)
        if n.shape != _nodes_shape(width, height):
            raise ValueError(f"the nodes must be int32 {_nodes_shape(width, height)}, got {n.shape}")
        keep += held + [t, n]
        for s in range(3):
            arr[k].image[s], arr[k].filled[s] = pi[s], pf[s]
        arr[k].lut, arr[k].nodes, arr[k].rows = t.ctypes.data, n.ctypes.data, rows
    out = np.zeros((height, width, planes), dtype=np.uint8)
    val, cov = np.zeros((height, width), dtype=np.uint8), np.zeros((height, width), dtype=np.uint8)
    check(lib().mdemod_mosaic_model_blend(arr, len(sources), sel, planes, _blend_mode(blend), int(width), int(height), out.ctypes.data,
                                          val.ctypes.data if valid else None, cov.ctypes.data if cover else None), "mdemod_mosaic_model_blend")
    extra = ([val] if valid else []) + ([cov] if cover else [])
    return (out, *extra) if extra else out


def model_host(passes, select=(2, 1, 0), **opts) -> Mosaic:
    """``mdemod_mosaic_compose_host`` with the model in the kernel's place (no device)."""
    return _compose(lib().mdemod_mosaic_model_host, "mdemod_mosaic_model_host", passes, select, (), opts)
