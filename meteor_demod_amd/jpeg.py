"""The JPEG encoder: include/meteor_demod_amd_jpeg.h over ctypes.

Baseline JPEG (SOF0, 8 bit, JFIF, 4:4:4, the standard Huffman tables, restart markers) of a grey or colour picture, made on the GPU:
``encode`` takes a numpy array (uploaded, ``mdemod_jpeg_encode_host``) or a uint8 torch tensor on the GPU (encoded where it lies,
``mdemod_jpeg_encode_device``) and returns the file's bytes, ``write`` puts them into a file, ``entropy`` runs the second stage alone
on coefficients.  ``model_*`` is the host model of csrc/jpeg_host.cpp, the kernels' specification.  This module keeps its own binding
tables, as every layer's does; ``_capi.bind`` applies them.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _capi, _encode
from ._capi import check

MAX_WIDTH, MAX_HEIGHT, MAX_RESTART, RESTART = 8192, 16384, 64, 32
HEAD = {1: 330, 3: 613}

_P = C.POINTER
_PICTURE = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_jpeg.h
SIGNATURES = {
    "mdemod_jpeg_bound": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mdemod_jpeg_entropy_bound": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "mdemod_jpeg_workspace": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mdemod_jpeg_entropy_workspace": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "mdemod_jpeg_encode_device": (C.c_int, _PICTURE + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mdemod_jpeg_entropy_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mdemod_jpeg_result": (C.c_int, [C.c_void_p, _P(C.c_uint64), C.c_int, C.c_void_p]),
    "mdemod_jpeg_encode_host": (C.c_int, _PICTURE + [_P(C.c_void_p), _P(C.c_uint64), C.c_int]),
    "mdemod_jpeg_free": (None, [C.c_void_p]),
}
# the host model (csrc/jpeg_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_jpeg_model_tables": (C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mdemod_jpeg_model_fdct": (None, [C.c_void_p, C.c_void_p]),
    "mdemod_jpeg_model_coefficients": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mdemod_jpeg_model_entropy": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "mdemod_jpeg_model_encode": (C.c_int, _PICTURE + [C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
}


@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


def _picture(picture) -> tuple:
    """(contiguous uint8 array, width, height, planes) of a numpy picture [H, W], [H, W, 1] or [H, W, 3]."""
    px, _, w, h, planes = _encode.picture(picture)
    return px, w, h, planes


def bound(width: int, height: int, planes: int, restart_interval: int = 0) -> int:
    """The largest file of such a picture (0: arguments out of range)."""
    return int(lib().mdemod_jpeg_bound(width, height, planes, restart_interval))


def workspace(width: int, height: int, planes: int, restart_interval: int = 0) -> int:
    return int(lib().mdemod_jpeg_workspace(width, height, planes, restart_interval))


# ------------------------------------------------------------------------------------------------------------------ device
def _first_room(w: int, h: int, planes: int, restart_interval: int) -> int:
    """The output buffer ``encode_tensor`` tries first: the bound (6.5 bytes a sample), but no more than twice the picture and 1 MiB."""
    return min(max(bound(w, h, planes, restart_interval), 1), 2 * w * h * planes + (1 << 20))


def encode_tensor(picture, quality: int = 90, restart_interval: int = 0, out_room: int | None = None) -> bytes:
    """A contiguous uint8 tensor [H, W], [H, W, 1] or [H, W, 3] on the GPU into the file's bytes, on the tensor's device and the
    current stream; only the file is downloaded.  ``out_room`` (default: the bound, at most twice the picture and 1 MiB) is the
    device buffer the file must fit; a ``MdemodError`` names the bytes needed when it does not."""
    w, h, planes = _encode.tensor(picture)
    need = workspace(w, h, planes, restart_interval)
    for attempt in range(2):
        room = int(out_room) if out_room is not None else _first_room(w, h, planes, restart_interval)
        s = _encode.Scratch(picture, room, need)
        check(lib().mdemod_jpeg_encode_device(C.c_void_p(picture.data_ptr()), w, h, planes, int(quality), int(restart_interval), *s.tail), "mdemod_jpeg_encode_device")
        try:
            return s.finish(lib().mdemod_jpeg_result, "mdemod_jpeg_result")
        except _capi.MdemodError as e:
            # a picture that codes to more than twice its size (noise at quality 100): once more with what it needs
            if out_room is not None or attempt or e.code != _capi.MDEMOD_ERR_OVERFLOW:
                raise
            out_room = int(s.result.cpu()[0])
    raise AssertionError("unreachable")


def entropy(coef, planes: int, restart_interval: int = 0, out_room: int | None = None) -> bytes:
    """The second stage alone: an int16 tensor [n_mcus * planes, 64] on the GPU (zig-zag order, the blocks of an MCU adjacent) into
    the segments and the markers between them."""
    import torch
    if coef.dtype != torch.int16 or not coef.is_contiguous() or coef.dim() != 2 or coef.shape[1] != 64 or coef.shape[0] % planes:
        raise ValueError("the coefficients must be a contiguous int16 tensor [n_mcus * planes, 64]")
    n_mcus = int(coef.shape[0]) // planes
    room = int(out_room) if out_room is not None else int(lib().mdemod_jpeg_entropy_bound(n_mcus, planes, restart_interval))
    s = _encode.Scratch(coef, room, int(lib().mdemod_jpeg_entropy_workspace(n_mcus, restart_interval)))
    check(lib().mdemod_jpeg_entropy_device(C.c_void_p(coef.data_ptr()), n_mcus, planes, int(restart_interval), *s.tail), "mdemod_jpeg_entropy_device")
    return s.finish(lib().mdemod_jpeg_result, "mdemod_jpeg_result")


def encode_host(picture, quality: int = 90, restart_interval: int = 0, device: int = 0) -> bytes:
    """``mdemod_jpeg_encode_host`` on a numpy picture."""
    px, w, h, planes = _picture(picture)
    return _encode.host_call(lib().mdemod_jpeg_encode_host, "mdemod_jpeg_encode_host", lib().mdemod_jpeg_free,
                             (px.ctypes.data, w, h, planes, int(quality), int(restart_interval)), device)


def encode(picture, quality: int = 90, restart_interval: int = 0, device: int = 0) -> bytes:
    """The JPEG file of ``picture``: a numpy array (uploaded to ``device``) or a uint8 tensor on the GPU (encoded where it lies)."""
    if isinstance(picture, np.ndarray):
        return encode_host(picture, quality, restart_interval, device)
    return encode_tensor(picture, quality, restart_interval)


def write(path, picture, quality: int = 90, restart_interval: int = 0, device: int = 0) -> int:
    """``encode`` into the file ``path``; returns the bytes written."""
    return _encode.write(path, encode(picture, quality, restart_interval, device))


# ------------------------------------------------------------------------------------------------------------- the host model
def model_tables(quality: int = 50):
    """(q[2][64] natural order, bits[4][16], vals[4][162], zigzag[64], m[8][8]) as the encoder holds them; tables 0 .. 3 are DC
    luminance, AC luminance, DC chrominance, AC chrominance."""
    q, bits, vals = np.zeros((2, 64), np.uint8), np.zeros((4, 16), np.uint8), np.zeros((4, 162), np.uint8)
    zigzag, m = np.zeros(64, np.uint8), np.zeros((8, 8), np.int32)
    check(lib().mdemod_jpeg_model_tables(int(quality), q.ctypes.data, bits.ctypes.data, vals.ctypes.data, zigzag.ctypes.data, m.ctypes.data), "mdemod_jpeg_model_tables")
    return q, bits, vals, zigzag, m


def model_fdct(samples) -> np.ndarray:
    """2^18 times the coefficients of one block of samples [8, 8] (uint8), natural order, int32."""
    s = np.ascontiguousarray(samples, dtype=np.uint8).reshape(64)
    out = np.zeros((8, 8), np.int32)
    lib().mdemod_jpeg_model_fdct(s.ctypes.data, out.ctypes.data)
    return out


def model_coefficients(picture, quality: int = 90) -> np.ndarray:
    """int16 [mcus * planes, 64]: the levels of the picture, zig-zag order."""
    px, w, h, planes = _picture(picture)
    coef = np.zeros((((w + 7) // 8) * ((h + 7) // 8) * planes, 64), np.int16)
    check(lib().mdemod_jpeg_model_coefficients(px.ctypes.data, w, h, planes, int(quality), coef.ctypes.data), "mdemod_jpeg_model_coefficients")
    return coef


def model_entropy(coef, planes: int, restart_interval: int = 0, out_room: int | None = None) -> bytes:
    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1, 64)
    n_mcus = coef.shape[0] // planes
    room = int(out_room) if out_room is not None else int(lib().mdemod_jpeg_entropy_bound(n_mcus, planes, restart_interval))
    out, n = np.zeros(max(room, 1), np.uint8), C.c_uint64()
    check(lib().mdemod_jpeg_model_entropy(coef.ctypes.data, n_mcus, planes, int(restart_interval), out.ctypes.data, room, C.byref(n)), "mdemod_jpeg_model_entropy")
    return out[: n.value].tobytes()


def model_encode(picture, quality: int = 90, restart_interval: int = 0, out_room: int | None = None) -> bytes:
    """``encode`` by the host model (``mdemod_jpeg_model_encode``; no device)."""
    px, w, h, planes = _picture(picture)
    room = int(out_room) if out_room is not None else bound(w, h, planes, restart_interval)
    out, n = np.zeros(max(room, 1), np.uint8), C.c_uint64()
    check(lib().mdemod_jpeg_model_encode(px.ctypes.data, w, h, planes, int(quality), int(restart_interval), out.ctypes.data, room, C.byref(n)), "mdemod_jpeg_model_encode")
    return out[: n.value].tobytes()
