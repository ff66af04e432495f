"""The equalise layer: include/meteor_demod_amd_equalise.h over ctypes.

Contrast-limited adaptive histogram equalisation (CLAHE) of a grey or colour picture on the GPU: ``apply`` takes a numpy array
(uploaded, ``mdemod_equalise_host``) or a uint8 torch tensor on the GPU (equalised where it lies, ``mdemod_equalise_device``) and
returns the same kind; ``tables`` returns the tables and counts the device made.  ``model_*`` is the host model of
csrc/equalise_host.cpp, the kernels' specification.  This module keeps its own binding tables, as every layer's does;
``_capi.bind`` applies them.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _capi
from ._capi import check

MAX_WIDTH, MAX_HEIGHT, MIN_TILE, MAX_TILE, MIN_CLIP, MAX_CLIP, MAX_AMOUNT = 8192, 16384, 16, 512, 100, 25600, 256
MODES = {"planes": 0, "luma": 1}


class Opts(C.Structure):
    _fields_ = [("tile", C.c_uint32), ("clip_percent", C.c_uint32), ("amount", C.c_uint32), ("mode", C.c_uint32), ("valid_step", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class Summary(C.Structure):
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("channels", C.c_uint32), ("empty_tiles", C.c_uint32)]


_P = C.POINTER
_PICTURE = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _P(Opts)]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_equalise.h
SIGNATURES = {
    "mdemod_equalise_default_opts": (None, [_P(Opts)]),
    "mdemod_equalise_workspace": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, _P(Opts)]),
    "mdemod_equalise_tables_device": (C.c_int, _PICTURE + [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mdemod_equalise_apply_device": (C.c_int, _PICTURE + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_equalise_device": (C.c_int, _PICTURE + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_equalise_host": (C.c_int, [_P(Opts), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _P(Summary), C.c_int]),
}
# the host model (csrc/equalise_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_equalise_model_table": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mdemod_equalise_model_tables": (C.c_int, _PICTURE + [C.c_void_p, C.c_uint64]),
    "mdemod_equalise_model_apply": (C.c_int, _PICTURE + [C.c_void_p, C.c_void_p]),
}


@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


def default_opts() -> Opts:
    o = Opts()
    lib().mdemod_equalise_default_opts(C.byref(o))
    return o


def options(tile: int = 128, clip: float = 3.0, amount: float = 1.0, mode="luma", valid_step: int = 1) -> Opts:
    """The options as the library takes them: ``clip`` in multiples of a flat histogram's count (round(100 clip) percent),
    ``amount`` 0 .. 1 (round(256 amount)), ``mode`` "luma" or "planes" (or 1, 0)."""
    o = Opts()
    o.tile, o.clip_percent, o.amount = int(tile), int(round(100.0 * clip)), int(round(256.0 * amount))
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"mode is 'luma' or 'planes', not {mode!r}")
        mode = MODES[mode]
    o.mode, o.valid_step = int(mode), int(valid_step)
    return o


def geometry(width: int, height: int, planes: int, opts: Opts) -> tuple:
    """(channels, ny, nx) of such a picture."""
    t = opts.tile
    channels = 3 if planes == 3 and opts.mode == 0 else 1
    return channels, max(1, (height + t // 2) // t), max(1, (width + t // 2) // t)


def workspace(width: int, height: int, planes: int, opts: Opts | None = None) -> int:
    """``mdemod_equalise_workspace`` (0: arguments out of range; opts None: the defaults)."""
    return int(lib().mdemod_equalise_workspace(int(width), int(height), int(planes), C.byref(opts) if opts is not None else None))


def _shape(shape) -> tuple:
    if len(shape) == 2:
        return int(shape[1]), int(shape[0]), 1
    if len(shape) == 3 and shape[2] in (1, 3):
        return int(shape[1]), int(shape[0]), int(shape[2])
    raise ValueError(f"a picture is uint8 [H, W] or [H, W, 3], got {tuple(shape)}")


def _mask(valid, w: int, h: int, step: int):
    if valid is None:
        return None
    rows = (h + step - 1) // step if step in (1, 8) else h
    if tuple(valid.shape) != (rows, w):
        raise ValueError(f"the mask of a {w} x {h} picture at valid_step {step} is uint8 [{rows}, {w}], got {tuple(valid.shape)}")
    return valid


def _split(work: np.ndarray, channels: int, ny: int, nx: int) -> tuple:
    n = channels * ny * nx
    return work[: n * 256].reshape(channels, ny, nx, 256).copy(), work[n * 256: n * 260].copy().view(np.uint32).reshape(channels, ny, nx)


# ------------------------------------------------------------------------------------------------------------------ device
def _tensor_args(picture, valid, opts: Opts):
    import torch
    if picture.dtype != torch.uint8 or not picture.is_contiguous() or not picture.is_cuda:
        raise ValueError("the picture must be a contiguous uint8 tensor on the GPU")
    w, h, planes = _shape(picture.shape)
    valid = _mask(valid, w, h, opts.valid_step)
    if valid is not None and (valid.dtype != torch.uint8 or not valid.is_contiguous() or valid.device != picture.device):
        raise ValueError("the mask must be a contiguous uint8 tensor on the picture's device")
    d = picture.device.index or 0
    stream = C.c_void_p(torch.cuda.current_stream(d).cuda_stream)
    need = workspace(w, h, planes, opts)
    work = torch.empty(max(need, 4), dtype=torch.uint8, device=picture.device)
    return w, h, planes, valid, d, stream, need, work


def apply_tensor(picture, valid=None, opts: Opts | None = None, out=None):
    """A contiguous uint8 tensor [H, W] or [H, W, 3] on the GPU through ``mdemod_equalise_device`` on its device and the current
    stream; ``out`` (default: a new tensor; may be ``picture`` itself) receives and is the result."""
    import torch
    opts = opts if opts is not None else default_opts()
    w, h, planes, valid, d, stream, need, work = _tensor_args(picture, valid, opts)
    if out is None:
        out = torch.empty_like(picture)
    check(lib().mdemod_equalise_device(C.c_void_p(picture.data_ptr()), C.c_void_p(valid.data_ptr()) if valid is not None else None, w, h, planes, C.byref(opts),
                                       C.c_void_p(work.data_ptr()), need, C.c_void_p(out.data_ptr()), d, stream), "mdemod_equalise_device")
    return out


def apply(picture, valid=None, tile: int = 128, clip: float = 3.0, amount: float = 1.0, mode="luma", valid_step: int = 1, device: int = 0):
    """The equalised picture: a numpy array (uploaded to ``device``; a new array comes back) or a uint8 tensor on the GPU (equalised
    where it lies into a new tensor)."""
    opts = options(tile, clip, amount, mode, valid_step)
    if not isinstance(picture, np.ndarray):
        return apply_tensor(picture, valid, opts)
    px = np.array(picture, dtype=np.uint8, order="C")
    w, h, planes = _shape(px.shape)
    mask = None if valid is None else np.ascontiguousarray(_mask(np.asarray(valid), w, h, opts.valid_step), dtype=np.uint8)
    check(lib().mdemod_equalise_host(C.byref(opts), px.ctypes.data, mask.ctypes.data if mask is not None else None, w, h, planes, None, int(device)), "mdemod_equalise_host")
    return px


def apply_host(picture, valid=None, opts: Opts | None = None, device: int = 0) -> tuple:
    """``mdemod_equalise_host`` on a copy of a numpy picture: (the result, its ``Summary``)."""
    opts = opts if opts is not None else default_opts()
    px = np.array(picture, dtype=np.uint8, order="C")
    w, h, planes = _shape(px.shape)
    mask = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    s = Summary()
    check(lib().mdemod_equalise_host(C.byref(opts), px.ctypes.data, mask.ctypes.data if mask is not None else None, w, h, planes, C.byref(s), int(device)), "mdemod_equalise_host")
    return px, s


def tables(picture, valid=None, tile: int = 128, clip: float = 3.0, amount: float = 1.0, mode="luma", valid_step: int = 1, device: int = 0) -> tuple:
    """(tab uint8 [channels, ny, nx, 256], count uint32 [channels, ny, nx]) as the device makes them, of a numpy array or a GPU tensor."""
    import torch
    opts = options(tile, clip, amount, mode, valid_step)
    if isinstance(picture, np.ndarray):
        picture = torch.from_numpy(np.ascontiguousarray(picture, dtype=np.uint8)).to(f"cuda:{int(device)}")
        valid = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8)).to(picture.device)
    w, h, planes, valid, d, stream, need, work = _tensor_args(picture, valid, opts)
    check(lib().mdemod_equalise_tables_device(C.c_void_p(picture.data_ptr()), C.c_void_p(valid.data_ptr()) if valid is not None else None, w, h, planes, C.byref(opts),
                                              C.c_void_p(work.data_ptr()), need, d, stream), "mdemod_equalise_tables_device")
    return _split(work.cpu().numpy(), *geometry(w, h, planes, opts))


# ------------------------------------------------------------------------------------------------------------- the host model
def model_table(hist, clip_percent: int = 300) -> tuple:
    """(n, h'' uint32 [256], tab uint8 [256]) of one histogram."""
    hist = np.ascontiguousarray(hist, dtype=np.uint32).reshape(256)
    h2, tab = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    n = lib().mdemod_equalise_model_table(hist.ctypes.data, int(clip_percent), h2.ctypes.data, tab.ctypes.data)
    return int(n), h2, tab


def model_workspace(picture, valid=None, opts: Opts | None = None) -> np.ndarray:
    """The public part of the workspace as the model fills it: uint8 [workspace]."""
    opts = opts if opts is not None else default_opts()
    px = np.ascontiguousarray(picture, dtype=np.uint8)
    w, h, planes = _shape(px.shape)
    mask = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    need = workspace(w, h, planes, opts)
    work = np.zeros(max(need, 4), np.uint8)
    check(lib().mdemod_equalise_model_tables(px.ctypes.data, mask.ctypes.data if mask is not None else None, w, h, planes, C.byref(opts), work.ctypes.data, need),
          "mdemod_equalise_model_tables")
    return work


def model_tables(picture, valid=None, tile: int = 128, clip: float = 3.0, amount: float = 1.0, mode="luma", valid_step: int = 1) -> tuple:
    """``tables`` by the host model (no device)."""
    opts = options(tile, clip, amount, mode, valid_step)
    w, h, planes = _shape(np.shape(picture))
    return _split(model_workspace(picture, valid, opts), *geometry(w, h, planes, opts))


def model_apply(picture, valid=None, tile: int = 128, clip: float = 3.0, amount: float = 1.0, mode="luma", valid_step: int = 1, work=None) -> np.ndarray:
    """``apply`` by the host model (no device); ``work``: a workspace to apply instead of the picture's own."""
    opts = options(tile, clip, amount, mode, valid_step)
    px = np.ascontiguousarray(picture, dtype=np.uint8)
    w, h, planes = _shape(px.shape)
    mask = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    work = model_workspace(px, mask, opts) if work is None else np.ascontiguousarray(work, dtype=np.uint8)
    out = np.zeros_like(px)
    check(lib().mdemod_equalise_model_apply(px.ctypes.data, mask.ctypes.data if mask is not None else None, w, h, planes, C.byref(opts), work.ctypes.data, out.ctypes.data),
          "mdemod_equalise_model_apply")
    return out
