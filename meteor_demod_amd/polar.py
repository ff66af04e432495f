"""The polar layer: include/meteor_demod_amd_polar.h over ctypes.

1 to 8 passes, each what ``mosaic.compose`` takes, on one polar stereographic grid.  ``grid`` makes the frame with every pass's solver
constants and host nodes, ``nodes_device`` solves the nodes on the GPU into device tensors, ``compose`` chains everything for numpy
arrays (through ``mdemod_polar_compose_host``, in bands) and ``images_to_polar`` takes a list of what ``image.vcdu_to_image``
returns.  ``graticule`` and ``vertices`` make what ``overlay`` cuts, bins and draws.  ``model_*`` is the host side alone: the map
layer's solver and the mosaic layer's model blend.  This module keeps its own binding tables, as every layer's does.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field

import numpy as np

from . import _capi, mosaic as _mosaic
from ._capi import check, take_bytes
from .map import _date, _packets
from .mosaic import Pass, PassRecord
from .picture import _SLOTS, _host_slots, _select, composite_select

MAX_PASSES = 8
FEATHER, BEST = 0, 1
BLENDS = {"feather": FEATHER, "best": BEST}
DATE_AUTO = -(1 << 31)
NO_NODE = -(1 << 31)
STEREOGRAPHIC = 0


class MdemodPolarOpts(C.Structure):
    _fields_ = [("scan_deg", C.c_double), ("time_offset", C.c_double), ("row_period", C.c_double), ("metres_per_pixel", C.c_double), ("lat_ts_deg", C.c_double),
                ("lon0_deg", C.c_double), ("side", C.c_int32), ("pole", C.c_int32), ("stretch", C.c_uint32), ("clip_low", C.c_uint32), ("clip_high", C.c_uint32),
                ("piece_lines", C.c_uint32), ("blend", C.c_uint32), ("nodes_on_host", C.c_uint32), ("projection", C.c_uint32), ("reserved", C.c_uint32)]


class MdemodPolarPass(C.Structure):
    _fields_ = [("tle_text", C.c_char_p), ("norad", C.c_uint32), ("date", C.c_int32), ("image", _SLOTS), ("filled", _SLOTS), ("rows", C.c_uint32),
                ("reserved", C.c_uint32), ("place", C.c_void_p), ("sinfo", C.c_void_p), ("n_desc", C.c_uint64)]


class MdemodPolarTiming(C.Structure):
    _fields_ = [("row_period", C.c_double), ("s0", C.c_double), ("date", C.c_int32), ("rows_fit", C.c_uint32), ("placed", C.c_uint32), ("lines", C.c_uint32)]


class MdemodPolarFrame(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("node_rows", C.c_uint32), ("node_cols", C.c_uint32), ("pole", C.c_int32), ("projection", C.c_uint32),
                ("res", C.c_double), ("e_left", C.c_double), ("n_top", C.c_double), ("lat_ts_deg", C.c_double), ("lon0_deg", C.c_double)]


class MdemodPolarSolver(C.Structure):
    _fields_ = [("a", C.c_double), ("cos_i", C.c_double), ("sin_i", C.c_double), ("raan", C.c_double), ("u", C.c_double), ("g", C.c_double), ("raan_rate", C.c_double),
                ("u_rate", C.c_double), ("g_rate", C.c_double), ("table_t0", C.c_double), ("sec_lo", C.c_double), ("sec_hi", C.c_double), ("theta_max", C.c_double),
                ("s0", C.c_double), ("line_period", C.c_double), ("time_offset", C.c_double), ("step", C.c_double), ("side", C.c_int32), ("table_n", C.c_uint32),
                ("table", C.c_void_p)]


class MdemodPolarNodes(C.Structure):
    _fields_ = [("frame", MdemodPolarFrame), ("n", C.c_uint32), ("reserved", C.c_uint32), ("timing", MdemodPolarTiming * MAX_PASSES),
                ("solver", MdemodPolarSolver * MAX_PASSES), ("nodes", C.c_void_p * MAX_PASSES)]


class MdemodPolarResult(C.Structure):
    _fields_ = [("frame", MdemodPolarFrame), ("planes", C.c_uint32), ("n", C.c_uint32), ("blend", C.c_uint32), ("nodes_on_host", C.c_uint32),
                ("timing", MdemodPolarTiming * MAX_PASSES), ("utc0", C.c_double * MAX_PASSES), ("lo", (C.c_uint32 * 3) * MAX_PASSES),
                ("hi", (C.c_uint32 * 3) * MAX_PASSES), ("covered", C.c_uint64 * MAX_PASSES), ("valid_pixels", C.c_uint64), ("overlap_pixels", C.c_uint64),
                ("pixels", C.c_void_p), ("valid", C.c_void_p), ("cover", C.c_void_p), ("nodes", C.c_void_p * MAX_PASSES)]


class MdemodPolarLines(C.Structure):
    _fields_ = [("lon", C.c_void_p), ("lat", C.c_void_p), ("first", C.c_void_p), ("n_lines", C.c_uint32), ("n_points", C.c_uint32), ("step_deg", C.c_double)]


class MdemodPolarPoints(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("first", C.c_void_p), ("n_lines", C.c_uint32), ("n_points", C.c_uint32)]


class MdemodPolarStyle(C.Structure):
    _fields_ = [("half_width", C.c_uint32), ("opacity", C.c_uint32), ("colour", C.c_uint8 * 3), ("inside_only", C.c_uint8)]


class MdemodPolarDrawn(C.Structure):
    _fields_ = [("pieces", C.c_uint64 * 4), ("tiles", C.c_uint64), ("items", C.c_uint64)]


_P = C.POINTER
_PROJ = [C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
_COMPOSE = [_P(MdemodPolarOpts), _P(MdemodPolarPass), C.c_uint32, C.c_void_p, C.c_uint32, _P(MdemodPolarResult)]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_polar.h
SIGNATURES = {
    "mdemod_polar_default_opts": (None, [_P(MdemodPolarOpts)]),
    "mdemod_polar_forward": (C.c_int, _PROJ),
    "mdemod_polar_inverse": (C.c_int, _PROJ),
    "mdemod_polar_grid": (C.c_int, [_P(MdemodPolarOpts), _P(MdemodPolarPass), C.c_uint32, _P(MdemodPolarNodes)]),
    "mdemod_polar_grid_free": (None, [_P(MdemodPolarNodes)]),
    "mdemod_polar_nodes_work_bytes": (C.c_uint64, [_P(MdemodPolarSolver), C.c_uint32]),
    "mdemod_polar_nodes_device": (C.c_int, [_P(MdemodPolarFrame), _P(MdemodPolarSolver), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mdemod_polar_compose_host": (C.c_int, _COMPOSE + [C.c_int]),
    "mdemod_polar_free": (None, [_P(MdemodPolarResult)]),
    "mdemod_polar_graticule": (C.c_int, [_P(MdemodPolarFrame), C.c_double, _P(MdemodPolarLines)]),
    "mdemod_polar_lines_free": (None, [_P(MdemodPolarLines)]),
    "mdemod_polar_vertices": (C.c_int, [_P(MdemodPolarFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, _P(MdemodPolarPoints)]),
    "mdemod_polar_points_free": (None, [_P(MdemodPolarPoints)]),
    "mdemod_polar_draw_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                         _P(MdemodPolarDrawn), C.c_int]),
    "mdemod_polar_world_file": (C.c_int, [_P(MdemodPolarFrame), C.c_char_p, C.c_uint64]),
    "mdemod_polar_prj": (C.c_int, [_P(MdemodPolarFrame), C.c_char_p, C.c_uint64]),
}
# the host side alone (csrc/polar_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_polar_model_nodes": (C.c_int, [_P(MdemodPolarOpts), _P(MdemodPolarPass), C.c_uint32, _P(MdemodPolarFrame), _P(MdemodPolarNodes)]),
    "mdemod_polar_model_host": (C.c_int, _COMPOSE),
}


@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed, and those of the layers under it (the same handle as ``_capi.lib()``)."""
    _mosaic.lib()
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


_FLOATS = ("scan_deg", "time_offset", "row_period", "metres_per_pixel", "lat_ts_deg", "lon0_deg")


def make_opts(**opts) -> MdemodPolarOpts:
    """``mdemod_polar_default_opts`` with the given fields replaced (an unknown name is a TypeError); ``blend`` may be "feather" or
    "best", ``lon0_deg`` None or "auto" for the pass's own."""
    o = MdemodPolarOpts()
    lib().mdemod_polar_default_opts(C.byref(o))
    names = {f[0] for f in MdemodPolarOpts._fields_} - {"reserved"}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"polar: no option {k!r} (there are: {', '.join(sorted(names))})")
        if k == "lon0_deg" and (v is None or v == "auto"):
            v = float("nan")
        setattr(o, k, float(v) if k in _FLOATS else BLENDS[v] if k == "blend" and isinstance(v, str) else int(v))
    return o


def _passes(passes):
    """The C array of the passes, and what must outlive the call."""
    arr, keep = (MdemodPolarPass * max(len(passes), 1))(), []
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


# ---------------------------------------------------------------------------------------------------------------- projection
def _project(entry, name, pole, lat_ts_deg, lon0_deg, a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    shape = a.shape
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    u, v = np.empty_like(a), np.empty_like(a)
    check(entry(int(pole), float(lat_ts_deg), float(lon0_deg), a.ctypes.data, b.ctypes.data, a.size, u.ctypes.data, v.ctypes.data), name)
    return u.reshape(shape), v.reshape(shape)


def forward(pole: int, lat_ts_deg: float, lon0_deg: float, lat, lon):
    """(lat, lon) in degrees to (E, N) in metres."""
    return _project(lib().mdemod_polar_forward, "mdemod_polar_forward", pole, lat_ts_deg, lon0_deg, lat, lon)


def inverse(pole: int, lat_ts_deg: float, lon0_deg: float, e, n):
    """(E, N) in metres to (lat, lon) in degrees, lon in -180 .. 180."""
    return _project(lib().mdemod_polar_inverse, "mdemod_polar_inverse", pole, lat_ts_deg, lon0_deg, e, n)


# --------------------------------------------------------------------------------------------------------------------- frame
@dataclass
class Frame:
    """Pixel (i, j) has its centre at ``e_left + (j + 0.5) res``, ``n_top - (i + 0.5) res`` metres; ``lat_ts_deg`` signed."""
    width: int
    height: int
    res: float
    e_left: float
    n_top: float
    pole: int
    lat_ts_deg: float
    lon0_deg: float

    @property
    def nodes_shape(self):
        return (-(-self.height // 16) + 1, -(-self.width // 16) + 1, 2)

    def c(self) -> MdemodPolarFrame:
        rows, cols, _ = self.nodes_shape
        return MdemodPolarFrame(int(self.width), int(self.height), rows, cols, int(self.pole), STEREOGRAPHIC, float(self.res), float(self.e_left), float(self.n_top),
                                float(self.lat_ts_deg), float(self.lon0_deg))

    def centres(self, i, j):
        """(E, N) of the centres of the pixels (i, j)."""
        return self.e_left + (np.asarray(j, dtype=np.float64) + 0.5) * self.res, self.n_top - (np.asarray(i, dtype=np.float64) + 0.5) * self.res

    def world_file(self) -> str:
        return world_file(self)

    def prj(self) -> str:
        return prj(self)


def _frame(f: MdemodPolarFrame) -> Frame:
    return Frame(int(f.width), int(f.height), float(f.res), float(f.e_left), float(f.n_top), int(f.pole), float(f.lat_ts_deg), float(f.lon0_deg))


def _text(entry, name, frame: Frame) -> str:
    buf = C.create_string_buffer(1024)
    f = frame.c()
    check(entry(C.byref(f), buf, len(buf)), name)
    return buf.value.decode("ascii")


def world_file(frame: Frame) -> str:
    """The six lines of the world file: res, 0, 0, -res, the centre of pixel (0, 0) in metres."""
    return _text(lib().mdemod_polar_world_file, "mdemod_polar_world_file", frame)


def prj(frame: Frame) -> str:
    """The WKT 1 text of the frame's projection."""
    return _text(lib().mdemod_polar_prj, "mdemod_polar_prj", frame)


# ---------------------------------------------------------------------------------------------------------------------- grid
@dataclass
class Solver:
    """What the node kernel is told of one pass: ``fields`` the numbers of ``mdemod_polar_solver`` by name, ``table`` float64
    [entries, 3]."""
    fields: dict
    table: np.ndarray

    def c(self) -> MdemodPolarSolver:
        s = MdemodPolarSolver()
        for k, v in self.fields.items():
            setattr(s, k, v)
        s.table_n, s.table = self.table.shape[0], self.table.ctypes.data
        return s


@dataclass
class Grid:
    """The frame with ``nodes`` int32 [passes, node rows, node cols, 2] solved on the host, the resolved line times and the solver
    constants of every pass."""
    frame: Frame
    nodes: np.ndarray
    passes: list
    solvers: list


def _record(t) -> PassRecord:
    return PassRecord(float(t.row_period), float(t.s0), int(t.rows_fit), int(t.placed), int(t.lines), int(t.date))


def _take_grid(g: MdemodPolarNodes) -> Grid:
    try:
        count = 8 * g.frame.node_rows * g.frame.node_cols
        nodes = np.stack([np.frombuffer(C.string_at(g.nodes[k], count), dtype=np.int32).reshape(g.frame.node_rows, g.frame.node_cols, 2) for k in range(g.n)])
        solvers = []
        for k in range(g.n):
            s = g.solver[k]
            fields = {name: getattr(s, name) for name, _ in MdemodPolarSolver._fields_ if name not in ("table", "table_n")}
            solvers.append(Solver(fields, np.frombuffer(C.string_at(s.table, 24 * s.table_n), dtype=np.float64).reshape(s.table_n, 3).copy()))
        return Grid(_frame(g.frame), nodes, [_record(g.timing[k]) for k in range(g.n)], solvers)
    finally:
        lib().mdemod_polar_grid_free(C.byref(g))


def grid(passes, **opts) -> Grid:
    """The frame of ``passes`` (a list of ``mosaic.Pass``) with every pass's host nodes, line times and solver constants."""
    o, g = make_opts(**opts), MdemodPolarNodes()
    arr, keep = _passes(passes)
    check(lib().mdemod_polar_grid(C.byref(o), arr, len(passes), C.byref(g)), "mdemod_polar_grid")
    return _take_grid(g)


def model_nodes(passes, frame: Frame, **opts) -> Grid:
    """``grid`` on a frame that is given: the host solver."""
    o, g, f = make_opts(**opts), MdemodPolarNodes(), frame.c()
    arr, keep = _passes(passes)
    check(lib().mdemod_polar_model_nodes(C.byref(o), arr, len(passes), C.byref(f), C.byref(g)), "mdemod_polar_model_nodes")
    return _take_grid(g)


def nodes_device(frame: Frame, solvers, device=None, out=None, work=None):
    """The nodes of every pass of ``solvers`` (a list of ``Solver``) on ``frame``, solved on the GPU: a list of int32
    [node rows, node cols, 2] device tensors, on the current stream.  ``out`` and ``work`` (a uint8 tensor) may be given."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    d = dev.index or 0
    f, n = frame.c(), len(solvers)
    arr = (MdemodPolarSolver * max(n, 1))(*[s.c() for s in solvers])
    if out is None:
        out = [torch.empty(frame.nodes_shape, dtype=torch.int32, device=dev) for _ in range(n)]
    for t in out:
        if t.dtype != torch.int32 or tuple(t.shape) != frame.nodes_shape or not t.is_contiguous():
            raise ValueError(f"the nodes must be contiguous int32 {frame.nodes_shape}")
    if work is None:
        work = torch.empty(max(int(lib().mdemod_polar_nodes_work_bytes(arr, n)), 8), dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in out])
    check(lib().mdemod_polar_nodes_device(C.byref(f), arr, n, ptrs, C.c_void_p(work.data_ptr()), work.numel(), d, C.c_void_p(torch.cuda.current_stream(d).cuda_stream)),
          "mdemod_polar_nodes_device")
    work.record_stream(torch.cuda.current_stream(d))
    return out


# ------------------------------------------------------------------------------------------------------------------- picture
@dataclass
class Polar:
    """``pixels`` uint8 [H, W] (grey) or [H, W, 3]; ``valid``, ``cover`` uint8 [H, W] as in ``mosaic.Mosaic``; ``nodes`` int32
    [passes, node rows, node cols, 2], the nodes the picture was made through; ``nodes_on_host`` where they were solved."""
    pixels: np.ndarray
    valid: np.ndarray
    cover: np.ndarray
    nodes: np.ndarray
    select: tuple
    frame: Frame
    blend: int
    nodes_on_host: bool
    passes: list = field(default_factory=list)
    valid_pixels: int = 0
    overlap_pixels: int = 0

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
        return world_file(self.frame)

    def prj(self) -> str:
        return prj(self.frame)


def _take(res: MdemodPolarResult, select) -> Polar:
    """A C result into arrays of our own; the C side's memory goes back."""
    try:
        f = _frame(res.frame)
        w, h, planes, n = f.width, f.height, int(res.planes), int(res.n)
        px = take_bytes(res.pixels, h * w * planes).reshape((h, w, planes) if planes == 3 else (h, w))
        records = []
        for k in range(n):
            r = _record(res.timing[k])
            r.utc0, r.covered = float(res.utc0[k]), int(res.covered[k])
            r.limits = [(int(res.lo[k][p]), int(res.hi[k][p])) for p in range(planes)]
            records.append(r)
        count = 8 * res.frame.node_rows * res.frame.node_cols
        nodes = np.stack([np.frombuffer(C.string_at(res.nodes[k], count), dtype=np.int32).reshape(f.nodes_shape) for k in range(n)])
        return Polar(px, take_bytes(res.valid, h * w).reshape(h, w), take_bytes(res.cover, h * w).reshape(h, w), nodes, tuple(int(s) for s in select), f,
                     int(res.blend), bool(res.nodes_on_host), records, int(res.valid_pixels), int(res.overlap_pixels))
    finally:
        lib().mdemod_polar_free(C.byref(res))


def _compose(entry, name, passes, select, tail, opts) -> Polar:
    o = make_opts(**opts)
    sel, planes = _select(select)
    arr, keep = _passes(passes)
    res = MdemodPolarResult()
    check(entry(C.byref(o), arr, len(passes), sel, planes, C.byref(res), *tail), name)
    return _take(res, select)


def compose(passes, select=(2, 1, 0), device: int = 0, **opts) -> Polar:
    """A list of ``mosaic.Pass`` (numpy arrays) to the finished ``Polar`` through ``mdemod_polar_compose_host`` (nodes on the GPU
    unless ``nodes_on_host=1``; bands of ``piece_lines``; ``device`` says where)."""
    return _compose(lib().mdemod_polar_compose_host, "mdemod_polar_compose_host", passes, select, (int(device),), opts)


def images_to_polar(results, tle_text, composite="auto", device: int = 0, norad: int = 0, date=None, **opts) -> Polar | None:
    """A list of ``image.Result`` (one per pass, all of the satellite of ``tle_text``) to a ``Polar``, as ``mosaic.images_to_mosaic``."""
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


def model_host(passes, select=(2, 1, 0), **opts) -> Polar:
    """``compose`` with host nodes and the mosaic layer's model blend (no device)."""
    return _compose(lib().mdemod_polar_model_host, "mdemod_polar_model_host", passes, select, (), opts)


# ------------------------------------------------------------------------------------------------------------------- vectors
def graticule(frame: Frame, step_deg: float = 0.0):
    """The graticule of a picture: (lon, lat, first, step) with float64 lon and lat in degrees and uint32 first [lines + 1]."""
    f, out = frame.c(), MdemodPolarLines()
    check(lib().mdemod_polar_graticule(C.byref(f), float(step_deg), C.byref(out)), "mdemod_polar_graticule")
    try:
        n, lines = int(out.n_points), int(out.n_lines)
        return (np.frombuffer(C.string_at(out.lon, 8 * n), dtype=np.float64).copy(), np.frombuffer(C.string_at(out.lat, 8 * n), dtype=np.float64).copy(),
                np.frombuffer(C.string_at(out.first, 4 * (lines + 1)), dtype=np.uint32).copy(), float(out.step_deg))
    finally:
        lib().mdemod_polar_lines_free(C.byref(out))


def vertices(frame: Frame, lon, lat, first):
    """Polylines in degrees to the overlay layer's fixed point on ``frame``: (x, y, first) with int32 x, y and uint32 first."""
    lon, lat = np.ascontiguousarray(lon, dtype=np.float64), np.ascontiguousarray(lat, dtype=np.float64)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    if first.size < 1 or lon.shape != lat.shape or lon.ndim != 1 or int(first[-1]) > lon.size:
        raise ValueError("lon and lat must be one-dimensional and alike, first [lines + 1] within them")
    f, out = frame.c(), MdemodPolarPoints()
    check(lib().mdemod_polar_vertices(C.byref(f), lon.ctypes.data, lat.ctypes.data, first.ctypes.data, first.size - 1, C.byref(out)), "mdemod_polar_vertices")
    try:
        n, lines = int(out.n_points), int(out.n_lines)
        return (np.frombuffer(C.string_at(out.x, 4 * n), dtype=np.int32).copy(), np.frombuffer(C.string_at(out.y, 4 * n), dtype=np.int32).copy(),
                np.frombuffer(C.string_at(out.first, 4 * (lines + 1)), dtype=np.uint32).copy())
    finally:
        lib().mdemod_polar_points_free(C.byref(out))


def draw(pixels, layers, styles, valid=None, device: int = 0):
    """``layers``: a list of ((x, y, first), style index) as ``vertices`` makes them; ``styles``: a list of (half_width, opacity,
    colour, inside_only) as the overlay layer takes them.  A copy of ``pixels`` (uint8 [H, W] or [H, W, 3]) with the lines on it,
    drawn on the GPU by the overlay layer's kernel, and the report (pieces per style, tiles, items)."""
    out = np.ascontiguousarray(pixels, dtype=np.uint8).copy()
    h, w, planes = out.shape[0], out.shape[1], (3 if out.ndim == 3 else 1)
    keep, pts = [], (MdemodPolarPoints * max(len(layers), 1))()
    for l, ((x, y, first), _) in enumerate(layers):
        x, y, first = np.ascontiguousarray(x, dtype=np.int32), np.ascontiguousarray(y, dtype=np.int32), np.ascontiguousarray(first, dtype=np.uint32)
        keep += [x, y, first]
        pts[l].x, pts[l].y, pts[l].first, pts[l].n_lines, pts[l].n_points = x.ctypes.data, y.ctypes.data, first.ctypes.data, first.size - 1, x.size
    ptrs = (C.c_void_p * max(len(layers), 1))(*[C.addressof(pts[l]) for l in range(len(layers))])
    style_of = (C.c_uint32 * max(len(layers), 1))(*[int(s) for _, s in layers])
    st = (MdemodPolarStyle * max(len(styles), 1))()
    for k, (half, opacity, colour, inside) in enumerate(styles):
        st[k].half_width, st[k].opacity, st[k].inside_only = int(half), int(opacity), int(bool(inside))
        for c in range(3):
            st[k].colour[c] = int(colour[c])
    val = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    rep = MdemodPolarDrawn()
    check(lib().mdemod_polar_draw_host(ptrs, style_of, len(layers), st, len(styles), w, h, planes, out.ctypes.data, None if val is None else val.ctypes.data,
                                       C.byref(rep), int(device)), "mdemod_polar_draw_host")
    return out, dict(pieces=[int(v) for v in rep.pieces], tiles=int(rep.tiles), items=int(rep.items))
