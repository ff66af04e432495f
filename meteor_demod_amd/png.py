"""The PNG encoder: include/meteor_demod_amd_png.h over ctypes.

Lossless PNG (8 bit, grey or RGB, the ``valid`` mask of a map as alpha; run matches at distance 1 and dynamic Huffman codes per
independent segment) made on the GPU: ``encode`` takes numpy arrays (uploaded, ``mdemod_png_encode_host``) or uint8 torch tensors on
the GPU (encoded where they lie, ``mdemod_png_encode_device``) and returns the file's bytes, ``write`` puts them into a file,
``deflate`` runs the second stage alone on any bytes.  ``model_*`` is the host model of csrc/png_host.cpp, the kernels'
specification.  This module keeps its own binding tables, as every layer's does; ``_capi.bind`` applies them.

    python -m meteor_demod_amd.png [--valid-from-black] a.ppm b.pgm ...

writes ``<name>.png`` beside each binary P5 / P6 file (maxval 255), so that a ``<name>.wld`` keeps matching.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from . import _capi, _encode
from ._capi import check
from ._encode import picture as _picture

MAX_WIDTH, MAX_HEIGHT, MAX_SEGMENT, FILTER_ADAPT = 8192, 16384, 32, 5
HEAD, TAIL, SEGMENT_OVERHEAD = 47, 28, 17

_P = C.POINTER
_PICTURE = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
_SIZE = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_png.h
SIGNATURES = {
    "mdemod_png_bound": (C.c_uint64, _SIZE),
    "mdemod_png_deflate_bound": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "mdemod_png_workspace": (C.c_uint64, _SIZE),
    "mdemod_png_deflate_workspace": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "mdemod_png_encode_device": (C.c_int, _PICTURE + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mdemod_png_deflate_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mdemod_png_result": (C.c_int, [C.c_void_p, _P(C.c_uint64), C.c_int, C.c_void_p]),
    "mdemod_png_encode_host": (C.c_int, _PICTURE + [_P(C.c_void_p), _P(C.c_uint64), C.c_int]),
    "mdemod_png_free": (None, [C.c_void_p]),
}
# the host model (csrc/png_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_png_model_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mdemod_png_model_deflate": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, _P(C.c_uint64), _P(C.c_uint64)]),
    "mdemod_png_model_encode": (C.c_int, _PICTURE + [C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
}


@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def channels(planes: int, has_valid: bool) -> int:
    return planes + (1 if has_valid else 0)


def bound(width: int, height: int, planes: int, has_valid: bool = False, segment: int = 0) -> int:
    """The largest file of such a picture (0: arguments out of range)."""
    return int(lib().mdemod_png_bound(width, height, planes, int(bool(has_valid)), segment))


def workspace(width: int, height: int, planes: int, has_valid: bool = False, segment: int = 0) -> int:
    return int(lib().mdemod_png_workspace(width, height, planes, int(bool(has_valid)), segment))


def deflate_bound(n_bytes: int, segment: int = 0) -> int:
    return int(lib().mdemod_png_deflate_bound(n_bytes, segment))


# ------------------------------------------------------------------------------------------------------------------ device
def encode_tensor(picture, valid=None, filter: int = FILTER_ADAPT, segment: int = 0, out_room: int | None = None) -> bytes:
    """A contiguous uint8 tensor [H, W], [H, W, 1] or [H, W, 3] on the GPU (and a mask [H, W] on the same device, or None) into the
    file's bytes, on the tensor's device and the current stream; only the file is downloaded.  ``out_room`` (default: the bound) is
    the device buffer the file must fit; a ``MdemodError`` names the bytes needed when it does not."""
    import torch
    w, h, planes = _encode.tensor(picture)
    if valid is not None and (valid.dtype != torch.uint8 or not valid.is_contiguous() or valid.device != picture.device or tuple(valid.shape) != (h, w)):
        raise ValueError("the mask must be a contiguous uint8 tensor [H, W] on the picture's device")
    need = workspace(w, h, planes, valid is not None, segment)
    room = int(out_room) if out_room is not None else bound(w, h, planes, valid is not None, segment)
    s = _encode.Scratch(picture, room, need)
    check(lib().mdemod_png_encode_device(C.c_void_p(picture.data_ptr()), C.c_void_p(valid.data_ptr()) if valid is not None else None, w, h, planes, int(filter),
                                         int(segment), *s.tail), "mdemod_png_encode_device")
    return s.finish(lib().mdemod_png_result, "mdemod_png_result")


def deflate(data, segment: int = 0, out_room: int | None = None) -> bytes:
    """The second stage alone: a contiguous uint8 tensor of any bytes on the GPU into the segments' IDAT chunks."""
    import torch
    if data.dtype != torch.uint8 or not data.is_contiguous() or not data.is_cuda or data.dim() != 1:
        raise ValueError("the bytes must be a contiguous one-dimensional uint8 tensor on the GPU")
    n = int(data.shape[0])
    room = int(out_room) if out_room is not None else deflate_bound(n, segment)
    s = _encode.Scratch(data, room, int(lib().mdemod_png_deflate_workspace(n, segment)))
    check(lib().mdemod_png_deflate_device(C.c_void_p(data.data_ptr()), n, int(segment), *s.tail), "mdemod_png_deflate_device")
    return s.finish(lib().mdemod_png_result, "mdemod_png_result")


def encode_host(picture, valid=None, filter: int = FILTER_ADAPT, segment: int = 0, device: int = 0) -> bytes:
    """``mdemod_png_encode_host`` on numpy arrays."""
    px, va, w, h, planes = _picture(picture, valid)
    return _encode.host_call(lib().mdemod_png_encode_host, "mdemod_png_encode_host", lib().mdemod_png_free,
                             (px.ctypes.data, _ptr(va), w, h, planes, int(filter), int(segment)), device)


def encode(picture, valid=None, filter: int = FILTER_ADAPT, segment: int = 0, device: int = 0) -> bytes:
    """The PNG file of ``picture`` (and ``valid`` as its alpha): numpy arrays (uploaded to ``device``) or uint8 tensors on the GPU
    (encoded where they lie)."""
    if isinstance(picture, np.ndarray):
        return encode_host(picture, valid, filter, segment, device)
    return encode_tensor(picture, valid, filter, segment)


def write(path, picture, valid=None, filter: int = FILTER_ADAPT, segment: int = 0, device: int = 0) -> int:
    """``encode`` into the file ``path``; returns the bytes written."""
    return _encode.write(path, encode(picture, valid, filter, segment, device))


# ------------------------------------------------------------------------------------------------------------- the host model
def model_filter(picture, valid=None, filter: int = FILTER_ADAPT) -> np.ndarray:
    """uint8 [height, 1 + width * channels]: the filtered stream, a row's filter byte first."""
    px, va, w, h, planes = _picture(picture, valid)
    out = np.zeros((h, 1 + w * channels(planes, va is not None)), np.uint8)
    check(lib().mdemod_png_model_filter(px.ctypes.data, _ptr(va), w, h, planes, int(filter), out.ctypes.data), "mdemod_png_model_filter")
    return out


def model_deflate(data, segment: int = 0, out_room: int | None = None, with_stored: bool = False):
    """The segments' IDAT chunks of any bytes by the host model; with ``with_stored`` also the number of stored segments."""
    b = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8).reshape(-1)
    room = int(out_room) if out_room is not None else deflate_bound(b.size, segment)
    out, n, stored = np.zeros(max(room, 1), np.uint8), C.c_uint64(), C.c_uint64()
    check(lib().mdemod_png_model_deflate(b.ctypes.data, b.size, int(segment), out.ctypes.data, room, C.byref(n), C.byref(stored)), "mdemod_png_model_deflate")
    return (out[: n.value].tobytes(), int(stored.value)) if with_stored else out[: n.value].tobytes()


def model_encode(picture, valid=None, filter: int = FILTER_ADAPT, segment: int = 0, out_room: int | None = None) -> bytes:
    """``encode`` by the host model (``mdemod_png_model_encode``; no device)."""
    px, va, w, h, planes = _picture(picture, valid)
    room = int(out_room) if out_room is not None else bound(w, h, planes, va is not None, segment)
    out, n = np.zeros(max(room, 1), np.uint8), C.c_uint64()
    check(lib().mdemod_png_model_encode(px.ctypes.data, _ptr(va), w, h, planes, int(filter), int(segment), out.ctypes.data, room, C.byref(n)), "mdemod_png_model_encode")
    return out[: n.value].tobytes()


# ------------------------------------------------------------------------------------------------------------- the command line
def read_pnm(path) -> np.ndarray:
    """A binary P5 ([H, W]) or P6 ([H, W, 3]) file with maxval 255."""
    with open(os.fspath(path), "rb") as f:
        data = f.read()
    fields, at = [], 0
    while len(fields) < 4:
        while at < len(data) and data[at : at + 1].isspace():
            at += 1
        if data[at : at + 1] == b"#":
            while at < len(data) and data[at] != 10:
                at += 1
            continue
        end = at
        while end < len(data) and not data[end : end + 1].isspace():
            end += 1
        if end == at:
            raise ValueError(f"{path}: the header ends early")
        fields.append(data[at:end])
        at = end
    at += 1                                                # the one white-space byte behind maxval
    if fields[0] not in (b"P5", b"P6"):
        raise ValueError(f"{path}: not a binary P5 / P6 file")
    w, h, maxval = (int(x) for x in fields[1:])
    if maxval != 255:
        raise ValueError(f"{path}: maxval {maxval}, only 255 is read")
    planes = 3 if fields[0] == b"P6" else 1
    if len(data) - at < w * h * planes:
        raise ValueError(f"{path}: {len(data) - at} bytes of pixels, {w * h * planes} are needed")
    px = np.frombuffer(data, np.uint8, w * h * planes, at)
    return px.reshape(h, w, 3) if planes == 3 else px.reshape(h, w)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m meteor_demod_amd.png", description="PNG files beside binary .pgm / .ppm files, made on the GPU")
    ap.add_argument("--valid-from-black", action="store_true", help="pixels whose planes are all 0 become transparent")
    ap.add_argument("--filter", type=int, default=FILTER_ADAPT, help="0 .. 4: one filter; 5: the least sum per row (default)")
    ap.add_argument("--segment", type=int, default=0, help="KiB per independent segment, 1 .. 32 (default 32)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("files", nargs="+")
    a = ap.parse_args(argv)
    for name in a.files:
        px = read_pnm(name)
        valid = None
        if a.valid_from_black:
            valid = (px.reshape(px.shape[0], px.shape[1], -1).max(axis=2) != 0).astype(np.uint8)
        out = os.path.splitext(name)[0] + ".png"
        n = write(out, px, valid, a.filter, a.segment, a.device)
        print(f"{out}: {px.shape[1]} x {px.shape[0]} x {px.shape[2] if px.ndim == 3 else 1}, {n} bytes out of {px.size} bytes in")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
