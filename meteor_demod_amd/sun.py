"""The sun layer: include/meteor_demod_amd_sun.h over ctypes.

The visible channels normalised by the sun's zenith angle, in the swath domain: ``position`` and ``cos_zenith`` are the astronomy,
``nodes`` the gain table of a pass, ``apply`` puts a table on channel pictures on the GPU (numpy arrays are uploaded, uint8 tensors
on the GPU are corrected where they lie), and ``correct`` takes what ``image.vcdu_to_image`` returns and gives back a copy with
corrected pictures that the picture, map, mosaic and polar layers take as it is.  ``model_apply`` is the host model of
csrc/sun_host.cpp, the kernel's specification.  This module keeps its own binding tables, as every layer's does; ``_capi.bind``
applies them.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np

from . import _capi
from . import map as _map
from ._capi import check
from .map import MdemodMapOpts, MdemodMapTiming, MdemodMapTle

NO_NODE = 0xFFFFFFFF
NODE_COLS, WIDTH, MAX_ROWS = 99, 1568, 8192
REFLECTIVE = (64, 65, 66)


class Opts(C.Structure):
    _fields_ = [("limit_deg", C.c_double), ("ref_deg", C.c_double), ("reserved", C.c_uint32 * 4)]


class Summary(C.Structure):
    _fields_ = [("zenith_min", C.c_double), ("zenith_max", C.c_double), ("nodes", C.c_uint32), ("missing", C.c_uint32), ("at_limit", C.c_uint32),
                ("slot_mask", C.c_uint32), ("date", C.c_int32), ("reserved", C.c_uint32), ("saturated", C.c_uint64 * 3)]


_P = C.POINTER
_SLOTS = C.c_void_p * 3
_CORRECT = [_P(Opts), _P(MdemodMapOpts), _P(MdemodMapTle), _P(_SLOTS), _P(C.c_uint32 * 3), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, _P(Summary)]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_sun.h
SIGNATURES = {
    "mdemod_sun_default_opts": (None, [_P(Opts)]),
    "mdemod_sun_position": (C.c_int, [C.c_int32, C.c_double, _P(C.c_double * 3)]),
    "mdemod_sun_cos_zenith": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mdemod_sun_nodes": (C.c_int, [_P(MdemodMapTle), _P(MdemodMapTiming), _P(MdemodMapOpts), _P(Opts), C.c_uint32, C.c_void_p, _P(Summary)]),
    "mdemod_sun_workspace": (C.c_uint64, [C.c_uint32]),
    "mdemod_sun_apply_device": (C.c_int, [_P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mdemod_sun_correct_host": (C.c_int, _CORRECT + [C.c_int]),
}
# the host model (csrc/sun_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_sun_model_apply": (C.c_int, [_P(_SLOTS), _P(_SLOTS), C.c_uint32, C.c_uint32, C.c_void_p, _P(C.c_uint64 * 3)]),
    "mdemod_sun_model_host": (C.c_int, _CORRECT),
}


@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed, and the map layer's, whose orbit and line times this layer works on
    (the same handle as ``_capi.lib()``)."""
    _map.lib()
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


def default_opts() -> Opts:
    o = Opts()
    lib().mdemod_sun_default_opts(C.byref(o))
    return o


def options(limit_deg: float | None = None, ref_deg: float | None = None) -> Opts:
    """``mdemod_sun_default_opts`` with the given angles replaced."""
    o = default_opts()
    if limit_deg is not None:
        o.limit_deg = float(limit_deg)
    if ref_deg is not None:
        o.ref_deg = float(ref_deg)
    return o


def _split_opts(opts: dict) -> tuple:
    """(sun options, map options) of one set of keywords: ``limit_deg`` and ``ref_deg`` are this layer's, the rest the map layer's."""
    opts = dict(opts)
    so = options(opts.pop("limit_deg", None), opts.pop("ref_deg", None))
    return so, _map.make_opts(**opts)


def summary_dict(s: Summary) -> dict:
    return {"zenith_min": float(s.zenith_min), "zenith_max": float(s.zenith_max), "nodes": int(s.nodes), "missing": int(s.missing), "at_limit": int(s.at_limit),
            "slot_mask": int(s.slot_mask), "date": int(s.date), "saturated": [int(v) for v in s.saturated]}


def workspace(rows: int) -> int:
    """``mdemod_sun_workspace`` (0: rows out of range)."""
    return int(lib().mdemod_sun_workspace(int(rows)))


def slot_mask(slots) -> int:
    """The mask of a sequence of slots (0 .. 2), or a mask as it is."""
    if isinstance(slots, (int, np.integer)):
        return int(slots)
    mask = 0
    for s in slots:
        if int(s) not in (0, 1, 2):
            raise ValueError(f"a slot is 0, 1 or 2, not {s!r}")
        mask |= 1 << int(s)
    return mask


# ------------------------------------------------------------------------------------------------------------------ astronomy
def position(date, utc: float) -> np.ndarray:
    """The Earth-fixed unit vector to the sun at second ``utc`` of day ``date`` (days since 1970-01-01, a ``datetime.date`` or
    "yyyy-mm-dd")."""
    out = (C.c_double * 3)()
    check(lib().mdemod_sun_position(_map._date(date), float(utc), C.byref(out)), "mdemod_sun_position")
    return np.array(out[:], dtype=np.float64)


def cos_zenith(date, utc, lat, lon) -> np.ndarray:
    """cos z at (``lat``, ``lon``) in degrees at the seconds ``utc`` of day ``date``; the three broadcast against each other."""
    u, la, lo = np.broadcast_arrays(np.asarray(utc, dtype=np.float64), np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    u, la, lo = (np.ascontiguousarray(v) for v in (u, la, lo))
    out = np.empty(u.shape)
    check(lib().mdemod_sun_cos_zenith(_map._date(date), u.ctypes.data, la.ctypes.data, lo.ctypes.data, u.size, out.ctypes.data), "mdemod_sun_cos_zenith")
    return out


def nodes(tle, timing: MdemodMapTiming, rows: int, norad: int = 0, **opts) -> tuple:
    """(gain uint32 [rows + 1, 99], summary dict) of a pass: ``opts`` are ``limit_deg``, ``ref_deg`` and the map layer's options."""
    so, mo = _split_opts(opts)
    s = Summary()
    gain = np.zeros((max(int(rows), 0) + 1, NODE_COLS), dtype=np.uint32)
    check(lib().mdemod_sun_nodes(C.byref(_map._tle(tle, norad)), C.byref(timing), C.byref(mo), C.byref(so), int(rows), gain.ctypes.data, C.byref(s)), "mdemod_sun_nodes")
    return gain, summary_dict(s)


# ---------------------------------------------------------------------------------------------------------------------- apply
def _rows_of(images, mask: int, is_fine) -> int:
    rows = None
    for k in range(3):
        if not (mask >> k & 1):
            continue
        im = images[k]
        if im is None or not is_fine(im):
            raise ValueError(f"the picture of slot {k} must be contiguous uint8 [8 rows, {WIDTH}]")
        if rows not in (None, im.shape[0] // 8):
            raise ValueError("the pictures differ in height")
        rows = im.shape[0] // 8
    if rows is None:
        raise ValueError("no slot selected")
    return rows


def apply_tensors(images, gain, slots=(0, 1, 2), out=None) -> tuple:
    """Uint8 [8 rows, 1568] tensors on the GPU (a sequence of three; the entries of slots that are not selected may be None) through
    ``mdemod_sun_apply_device`` on their device and the current stream.  ``out``: a like sequence that receives the selected slots
    (default: new tensors; an entry may be the picture itself).  (the list of outputs - unselected entries as given -, the partial
    counts as a uint32 [rows, 3] tensor)."""
    import torch
    mask = slot_mask(slots)
    rows = _rows_of(images, mask, lambda t: t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] == WIDTH and t.shape[0] % 8 == 0 and t.is_contiguous())
    dev = next(images[k].device for k in range(3) if mask >> k & 1)
    d = dev.index or 0
    if isinstance(gain, np.ndarray):
        gain = torch.from_numpy(np.ascontiguousarray(gain, dtype=np.uint32).view(np.int32)).to(dev)
    if gain.dtype != torch.int32 or tuple(gain.shape) != (rows + 1, NODE_COLS) or not gain.is_contiguous():
        raise ValueError(f"the gain table must be uint32 (numpy) or int32 (a tensor holding the same words) [{rows + 1}, {NODE_COLS}], got {gain.dtype} {tuple(gain.shape)}")
    outs = list(out) if out is not None else [None, None, None]
    pi, po = _SLOTS(), _SLOTS()
    for k in range(3):
        if not (mask >> k & 1):
            continue
        if outs[k] is None:
            outs[k] = torch.empty_like(images[k])
        if outs[k].dtype != torch.uint8 or tuple(outs[k].shape) != tuple(images[k].shape) or not outs[k].is_contiguous() or outs[k].device != dev:
            raise ValueError(f"the output of slot {k} must be a tensor like its picture")
        pi[k], po[k] = images[k].data_ptr(), outs[k].data_ptr()
    need = workspace(rows)
    work = torch.zeros((max(rows, 1), 3), dtype=torch.int32, device=dev)
    check(lib().mdemod_sun_apply_device(C.byref(pi), C.byref(po), mask, rows, C.c_void_p(gain.data_ptr()), C.c_void_p(work.data_ptr()), need, d,
                                        C.c_void_p(torch.cuda.current_stream(d).cuda_stream)), "mdemod_sun_apply_device")
    return outs, work


def apply(images, gain, slots=(0, 1, 2), out=None, device: int = 0) -> tuple:
    """The selected slots through the gain table on the GPU: (the pictures, saturated [3]).  ``images``: three numpy arrays (uploaded
    to ``device``; new arrays come back, the slots that are not selected as given) or three uint8 tensors on the GPU (``out=`` as
    ``apply_tensors`` takes it)."""
    import torch
    mask = slot_mask(slots)
    if any(isinstance(images[k], np.ndarray) for k in range(3) if mask >> k & 1):
        dev = f"cuda:{int(device)}"
        up = [torch.from_numpy(np.ascontiguousarray(images[k], dtype=np.uint8)).to(dev) if mask >> k & 1 else None for k in range(3)]
        outs, work = apply_tensors(up, np.asarray(gain), mask, out=up)
        res = [outs[k].cpu().numpy() if mask >> k & 1 else images[k] for k in range(3)]
        if out is not None:
            for k in range(3):
                if mask >> k & 1:
                    out[k][...] = res[k]
                    res[k] = out[k]
    else:
        res, work = apply_tensors(images, gain, mask, out=out)
    return res, [int(v) for v in work.to(torch.int64).sum(dim=0).cpu()]


def model_apply(images, gain, slots=(0, 1, 2)) -> tuple:
    """``apply`` by the host model (no device), numpy arrays in and out."""
    mask = slot_mask(slots)
    ims = [np.ascontiguousarray(images[k], dtype=np.uint8) if mask >> k & 1 else None for k in range(3)]
    rows = _rows_of(ims, mask, lambda a: a.ndim == 2 and a.shape[1] == WIDTH and a.shape[0] % 8 == 0)
    g = np.ascontiguousarray(gain, dtype=np.uint32)
    if g.shape != (rows + 1, NODE_COLS):
        raise ValueError(f"the gain table must be uint32 [{rows + 1}, {NODE_COLS}], got {g.shape}")
    outs = [np.zeros_like(ims[k]) if mask >> k & 1 else images[k] for k in range(3)]
    pi, po, sat = _SLOTS(), _SLOTS(), (C.c_uint64 * 3)()
    for k in range(3):
        if mask >> k & 1:
            pi[k], po[k] = ims[k].ctypes.data, outs[k].ctypes.data
    check(lib().mdemod_sun_model_apply(C.byref(pi), C.byref(po), mask, rows, g.ctypes.data, C.byref(sat)), "mdemod_sun_model_apply")
    return outs, [int(v) for v in sat]


# -------------------------------------------------------------------------------------------------------------------- correct
def _correct(entry, name, tail, images, apids, place, sinfo, tle, so, mo) -> tuple:
    ims = [np.array(im, dtype=np.uint8, order="C") for im in images]
    if len(ims) != 3 or any(im.ndim != 2 or im.shape[1] != WIDTH or im.shape != ims[0].shape or im.shape[0] % 8 for im in ims):
        raise ValueError(f"three pictures uint8 [8 rows, {WIDTH}] of one height are needed")
    p, s = _map._packets(place, sinfo)
    pi, ids, summ = _SLOTS(), (C.c_uint32 * 3)(*[int(a) for a in apids]), Summary()
    for k in range(3):
        pi[k] = ims[k].ctypes.data if ims[k].size else None
    check(entry(C.byref(so), C.byref(mo), C.byref(tle), C.byref(pi), C.byref(ids), ims[0].shape[0] // 8, p.ctypes.data if p.size else None,
                s.ctypes.data if s.size else None, p.size, C.byref(summ), *tail), name)
    return ims, summary_dict(summ)


def correct_images(images, apids, place, sinfo, tle, norad: int = 0, device: int = 0, model: bool = False, **opts) -> tuple:
    """``mdemod_sun_correct_host`` on copies of three numpy pictures: (the pictures, the summary dict).  ``model``: the host model in
    the kernel's place (no device)."""
    so, mo = _split_opts(opts)
    if model:
        return _correct(lib().mdemod_sun_model_host, "mdemod_sun_model_host", (), images, apids, place, sinfo, _map._tle(tle, norad), so, mo)
    return _correct(lib().mdemod_sun_correct_host, "mdemod_sun_correct_host", (int(device),), images, apids, place, sinfo, _map._tle(tle, norad), so, mo)


def correct(result, tle_text, norad: int = 0, slots=None, device: int = 0, **opts):
    """A copy of an ``image.Result`` whose ``images`` are corrected and which carries the summary dict as ``.sun``: what
    ``picture.image_to_picture``, ``map.image_to_map``, ``mosaic.images_to_mosaic`` and ``polar.images_to_polar`` take in the
    result's place.  The slots whose APID is 64, 65 or 66 are corrected, or the ``slots`` given (0 .. 2, in the order of the result's
    APIDs); ``opts`` are ``limit_deg``, ``ref_deg`` and the map layer's options (the ones the map is then made with)."""
    apids = list(result.images)
    if len(apids) != 3:
        raise ValueError("a result with three channels is needed")
    ids = list(apids) if slots is None else [REFLECTIVE[0] if slot_mask(slots) >> k & 1 else 0 for k in range(3)]
    ims, summ = correct_images([result.images[a] for a in apids], ids, result.place, result.sinfo, tle_text, norad=norad, device=device, **opts)
    out = dataclasses.replace(result, images={a: ims[k] for k, a in enumerate(apids)}, filled=dict(result.filled))
    out.sun = summ
    return out
