"""The picture layer: include/meteor_demod_amd_picture.h over ctypes.

``column_map`` gives the table that resamples a scan line to equal ground distance, ``histogram`` counts the filled pixels of the
three slots on the GPU, ``lut`` turns one histogram into a contrast table, ``render`` makes the grey or colour picture on the GPU
(device tensors in and out); ``compose`` chains them for numpy arrays (through ``mdemod_picture_compose_host``, in pieces) or device
tensors, and ``image_to_picture`` takes what ``image.vcdu_to_image`` returns.  ``model_*`` is the host model of
csrc/picture_host.cpp, the kernels' specification.  This module keeps its own binding table, as ``image.py`` does.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import check, take_bytes

SRC_WIDTH, CELLS = 1568, 14


class MdemodPictureOpts(C.Structure):
    _fields_ = [("altitude_km", C.c_double), ("scan_deg", C.c_double), ("rectify", C.c_uint32), ("stretch", C.c_uint32), ("clip_low", C.c_uint32),
                ("clip_high", C.c_uint32), ("piece_rows", C.c_uint32), ("reserved", C.c_uint32)]


class MdemodPictureResult(C.Structure):
    _fields_ = [("width", C.c_uint32), ("lines", C.c_uint32), ("planes", C.c_uint32), ("reserved", C.c_uint32), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3),
                ("valid_cells", C.c_uint64), ("pixels", C.c_void_p), ("valid", C.c_void_p)]


_P = C.POINTER
_SLOTS = C.c_void_p * 3
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_picture.h
SIGNATURES = {
    "mdemod_picture_default_opts": (None, [_P(MdemodPictureOpts)]),
    "mdemod_picture_column_map": (C.c_int, [_P(MdemodPictureOpts), C.c_void_p, C.c_uint32, _P(C.c_uint32)]),
    "mdemod_picture_histogram_device": (C.c_int, [_P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_picture_lut": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mdemod_picture_render_device": (C.c_int, [_P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_picture_compose_host": (C.c_int, [_P(MdemodPictureOpts), _P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p, C.c_uint32, _P(MdemodPictureResult),
                                              C.c_int]),
    "mdemod_picture_free": (None, [_P(MdemodPictureResult)]),
}
# the host model (csrc/picture_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_picture_model_histogram": (C.c_int, [_P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p]),
    "mdemod_picture_model_render": (C.c_int, [_P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_void_p]),
    "mdemod_picture_model_host": (C.c_int, [_P(MdemodPictureOpts), _P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_void_p, C.c_uint32, _P(MdemodPictureResult)]),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


def make_opts(**opts) -> MdemodPictureOpts:
    """``mdemod_picture_default_opts`` with the given fields replaced (an unknown name is a TypeError)."""
    o = MdemodPictureOpts()
    lib().mdemod_picture_default_opts(C.byref(o))
    names = {f[0] for f in MdemodPictureOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"picture: no option {k!r} (there are: {', '.join(sorted(names))})")
        setattr(o, k, float(v) if k in ("altitude_km", "scan_deg") else int(v))
    return o


@dataclass
class Picture:
    """``pixels`` uint8 [lines, width] (grey) or [lines, width, 3]; ``valid`` uint8 [lines / 8, width], bit p: plane p had a filled
    tap; ``limits`` the (lo, hi) of each plane's stretch; ``select`` the slot of each plane."""
    pixels: np.ndarray
    valid: np.ndarray
    limits: list
    select: tuple

    @property
    def width(self) -> int:
        return int(self.pixels.shape[1])

    @property
    def valid_share(self) -> float:
        return float(np.count_nonzero(self.valid)) / self.valid.size if self.valid.size else 0.0


def column_map(**opts) -> np.ndarray:
    """The column map of the options: uint32 [W]."""
    o = make_opts(**opts)
    w = C.c_uint32(0)
    check(lib().mdemod_picture_column_map(C.byref(o), None, 0, C.byref(w)), "mdemod_picture_column_map")
    out = np.zeros(w.value, dtype=np.uint32)
    check(lib().mdemod_picture_column_map(C.byref(o), out.ctypes.data, out.size, C.byref(w)), "mdemod_picture_column_map")
    return out


def lut(hist, clip_low: int = 5, clip_high: int = 5, stretch: bool = True, limits: bool = False):
    """The table of one histogram ([256] counts): uint8 [256]; with ``limits`` also (lo, hi).  ``stretch=False``: the identity."""
    if not stretch:
        table, lim = np.arange(256, dtype=np.uint8), (0, 255)
    else:
        h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(256)
        table, lim2 = np.zeros(256, dtype=np.uint8), np.zeros(2, dtype=np.uint32)
        check(lib().mdemod_picture_lut(h.ctypes.data, int(clip_low), int(clip_high), table.ctypes.data, lim2.ctypes.data), "mdemod_picture_lut")
        lim = (int(lim2[0]), int(lim2[1]))
    return (table, lim) if limits else table


def _select(select, planes=None):
    s = [int(x) for x in select]
    if planes is not None and len(s) != planes:
        raise ValueError(f"{len(s)} slots selected for {planes} planes")
    return (C.c_uint32 * len(s))(*s), len(s)


def _dev_slots(images, filled):
    """Three device pictures / masks (a [3, ...] tensor or a sequence, entries may be None) as pointer arrays; (device, rows)."""
    import torch
    pi, pf, rows, dev, keep = _SLOTS(), _SLOTS(), None, None, []
    for s in range(3):
        im, fl = images[s], filled[s]
        if im is None:
            continue
        if not im.is_cuda or im.dtype != torch.uint8 or im.dim() != 2 or im.shape[1] != SRC_WIDTH or im.shape[0] % 8:
            raise ValueError(f"a picture must be a uint8 [8 rows, 1568] device tensor, got {im.dtype} {tuple(im.shape)}")
        if fl.dtype == torch.bool:
            fl = fl.to(torch.uint8)
        im, fl = im.contiguous(), fl.contiguous()
        r = int(im.shape[0]) // 8
        if not fl.is_cuda or fl.dtype != torch.uint8 or tuple(fl.shape) != (r, CELLS):
            raise ValueError(f"a mask must be a uint8 or bool [rows, 14] device tensor, got {fl.dtype} {tuple(fl.shape)}")
        if rows not in (None, r):
            raise ValueError("the pictures differ in height")
        rows, dev = r, im.device
        keep += [im, fl]
        pi[s], pf[s] = (im.data_ptr() or None), (fl.data_ptr() or None)
    if rows is None:
        raise ValueError("no picture given")
    return pi, pf, rows, dev, keep


def histogram(images, filled):
    """uint8 [8 rows, 1568] pictures and [rows, 14] masks of the three slots (device tensors; a slot may be None) to the counts of
    the filled pixels: an int32 [3, 256] device tensor (the counts are below 2^32: read it as uint32).  On the current stream."""
    import torch
    pi, pf, rows, dev, keep = _dev_slots(images, filled)
    hist = torch.empty((3, 256), dtype=torch.int32, device=dev)
    d = dev.index or 0
    check(lib().mdemod_picture_histogram_device(C.byref(pi), C.byref(pf), rows, C.c_void_p(hist.data_ptr()), d,
                                                C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "mdemod_picture_histogram_device")
    return hist


def render(images, filled, select, luts, cmap, valid: bool = False):
    """The slots ``select`` (1 or 3 of them) through the tables ``luts`` (uint8 [planes, 256]) and the map ``cmap`` (uint32 / int32
    [W]) into a uint8 [8 rows, W, planes] device tensor; with ``valid`` also the uint8 [rows, W] one.  ``luts`` and ``cmap`` may be
    numpy arrays (copied to the device) or device tensors.  On the current stream."""
    import torch
    sel, planes = _select(select)
    chosen = [images[s] if s in select else None for s in range(3)]
    pi, pf, rows, dev, keep = _dev_slots(chosen, filled)
    d = dev.index or 0
    if isinstance(luts, np.ndarray):
        luts = torch.from_numpy(np.ascontiguousarray(luts, dtype=np.uint8)).to(dev)
    if isinstance(cmap, np.ndarray):
        cmap = torch.from_numpy(np.ascontiguousarray(cmap, dtype=np.uint32).view(np.int32)).to(dev)
    luts, cmap = luts.contiguous(), cmap.contiguous()
    if luts.dtype != torch.uint8 or luts.numel() != 256 * planes:
        raise ValueError(f"the tables must be uint8 [{planes}, 256]")
    if cmap.element_size() != 4 or cmap.dim() != 1:
        raise ValueError("the map must be a one-dimensional tensor of 32-bit words")
    width = int(cmap.numel())
    out = torch.empty((8 * rows, width, planes), dtype=torch.uint8, device=dev)
    val = torch.empty((rows, width), dtype=torch.uint8, device=dev) if valid else None
    check(lib().mdemod_picture_render_device(C.byref(pi), C.byref(pf), rows, sel, planes, C.c_void_p(luts.data_ptr()), C.c_void_p(cmap.data_ptr()), width,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(val.data_ptr()) if valid else None, d,
                                             C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "mdemod_picture_render_device")
    return (out, val) if valid else out


def _host_slots(images, filled):
    pi, pf, rows, keep = _SLOTS(), _SLOTS(), None, []
    for s in range(3):
        if images[s] is None:
            continue
        im = np.ascontiguousarray(images[s], dtype=np.uint8)
        if im.ndim != 2 or im.shape[1] != SRC_WIDTH or im.shape[0] % 8:
            raise ValueError(f"a picture must be uint8 [8 rows, 1568], got {im.shape}")
        r = im.shape[0] // 8
        fl = np.asarray(filled[s])
        fl = np.ascontiguousarray(fl if fl.dtype == np.uint8 else fl != 0, dtype=np.uint8)
        if fl.shape != (r, CELLS):
            raise ValueError(f"a mask must be [rows, 14], got {fl.shape}")
        if rows not in (None, r):
            raise ValueError("the pictures differ in height")
        rows = r
        keep += [im, fl]
        pi[s], pf[s] = (im.ctypes.data if im.size else None), (fl.ctypes.data if fl.size else None)
    if rows is None:
        raise ValueError("no picture given")
    return pi, pf, rows, keep


def _take(res: MdemodPictureResult, select) -> Picture:
    """A C result into arrays of our own; the C side's memory goes back."""
    try:
        w, lines, planes = int(res.width), int(res.lines), int(res.planes)
        px = take_bytes(res.pixels, lines * w * planes).reshape((lines, w, planes) if planes == 3 else (lines, w))
        return Picture(px, take_bytes(res.valid, lines // 8 * w).reshape(lines // 8, w), [(int(res.lo[p]), int(res.hi[p])) for p in range(planes)], tuple(select))
    finally:
        lib().mdemod_picture_free(C.byref(res))


def compose(images, filled, select=(2, 1, 0), device: int = 0, **opts) -> Picture:
    """Pictures and masks of the three slots to the finished ``Picture``.  numpy arrays go through ``mdemod_picture_compose_host``
    (copied in pieces of ``piece_rows``; ``device`` says where); device tensors through ``histogram``, ``lut`` and ``render`` on
    their device.  ``select`` names the slot of each plane: one for grey, three for R, G, B."""
    o = make_opts(**opts)
    sel, planes = _select(select)
    first = next(x for x in images if x is not None)
    if isinstance(first, np.ndarray):
        pi, pf, rows, keep = _host_slots(images, filled)
        res = MdemodPictureResult()
        check(lib().mdemod_picture_compose_host(C.byref(o), C.byref(pi), C.byref(pf), rows, sel, planes, C.byref(res), int(device)), "mdemod_picture_compose_host")
        return _take(res, select)
    chosen = [images[s] if s in select else None for s in range(3)]
    cmap = column_map(**{k: v for k, v in opts.items() if k != "piece_rows"})
    hist = histogram(chosen, filled).cpu().numpy().view(np.uint32) if o.stretch else np.zeros((3, 256), np.uint32)
    tables = [lut(hist[s], o.clip_low, o.clip_high, bool(o.stretch), limits=True) for s in select]
    out, val = render(chosen, filled, select, np.stack([t for t, _ in tables]), cmap, valid=True)
    px = out.cpu().numpy()
    return Picture(px if planes == 3 else px[:, :, 0], val.cpu().numpy(), [lim for _, lim in tables], tuple(int(s) for s in select))


def composite_select(composite, received) -> tuple | None:
    """``composite``: three digits 1 .. 3 (the slots of R, G, B, counted from 1), one digit (grey), or "auto": 321 when all three
    slots received a strip, 221 when only the first two did, otherwise None (no composite)."""
    text = str(composite)
    if text == "auto":
        got = [bool(x) for x in received]
        text = "321" if all(got) else "221" if got[0] and got[1] and not got[2] else ""
        if not text:
            return None
    if len(text) not in (1, 3) or any(c not in "123" for c in text):
        raise ValueError(f"composite {composite!r}: three digits 1 .. 3 (or one), or auto")
    return tuple(int(c) - 1 for c in text)


def image_to_picture(result, composite="auto", device: int = 0, **opts) -> Picture | None:
    """An ``image.Result`` to a ``Picture``: the slots are the result's channels in the order of its APIDs."""
    apids = list(result.images)
    images, filled = [result.images[a] for a in apids], [result.filled[a] for a in apids]
    select = composite_select(composite, [f.any() for f in filled])
    if select is None:
        return None
    return compose(images, filled, select, device=device, **opts)


# ------------------------------------------------------------------------------------------------------------- the host model
def model_histogram(images, filled) -> np.ndarray:
    pi, pf, rows, keep = _host_slots(images, filled)
    hist = np.zeros((3, 256), dtype=np.uint32)
    check(lib().mdemod_picture_model_histogram(C.byref(pi), C.byref(pf), rows, hist.ctypes.data), "mdemod_picture_model_histogram")
    return hist


def model_render(images, filled, select, luts, cmap, valid: bool = False):
    """(uint8 [8 rows, W, planes], and with ``valid`` uint8 [rows, W]) of the host model."""
    sel, planes = _select(select)
    pi, pf, rows, keep = _host_slots(images, filled)
    t = np.ascontiguousarray(luts, dtype=np.uint8).reshape(planes, 256)
    m = np.ascontiguousarray(cmap, dtype=np.uint32)
    out = np.zeros((8 * rows, m.size, planes), dtype=np.uint8)
    val = np.zeros((rows, m.size), dtype=np.uint8)
    check(lib().mdemod_picture_model_render(C.byref(pi), C.byref(pf), rows, sel, planes, t.ctypes.data, m.ctypes.data, m.size, out.ctypes.data,
                                            val.ctypes.data if valid else None), "mdemod_picture_model_render")
    return (out, val) if valid else out


def model_host(images, filled, select=(2, 1, 0), **opts) -> Picture:
    """``mdemod_picture_compose_host`` with the model in the kernels' place (no device): the pieces and the tables."""
    o = make_opts(**opts)
    sel, planes = _select(select)
    pi, pf, rows, keep = _host_slots(images, filled)
    res = MdemodPictureResult()
    check(lib().mdemod_picture_model_host(C.byref(o), C.byref(pi), C.byref(pf), rows, sel, planes, C.byref(res)), "mdemod_picture_model_host")
    return _take(res, select)
