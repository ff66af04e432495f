"""The transfer-frame layer: include/meteor_demod_amd_rs.h over ctypes.

``decode`` takes CADUs (1024 bytes each) to VCDUs (892 bytes each): the randomiser's sequence off, the four interleaved
Reed-Solomon (255,223) codewords corrected on the GPU, and per frame how many bytes each codeword needed (255: beyond the code).
A device tensor stays on the device; a numpy array goes through the host entry, copied in pieces.  ``decode_file`` reads a
``.cadu`` file, ``soft_to_vcdu`` chains the frame layer and this one without leaving the device.  ``model_*`` is the host model of
csrc/rs_host.cpp, the kernel's specification.  This module keeps its own binding table, as ``frames.py`` does.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import check

CADU_BYTES, VCDU_BYTES, T, FAILED, UNCORRECTABLE = 1024, 892, 16, 255, 1


class MdemodRsOpts(C.Structure):
    _fields_ = [("derandomise", C.c_uint32), ("dual_basis", C.c_uint32), ("piece_frames", C.c_uint64)]


class MdemodRsInfo(C.Structure):
    _fields_ = [("corrected", C.c_uint8 * 4), ("flags", C.c_uint32)]


class MdemodRsHeader(C.Structure):
    _fields_ = [("version", C.c_uint32), ("spacecraft", C.c_uint32), ("vcid", C.c_uint32), ("counter", C.c_uint32)]


_P = C.POINTER
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_rs.h
SIGNATURES = {
    "mdemod_rs_default_opts": (None, [_P(MdemodRsOpts)]),
    "mdemod_rs_decode_device": (C.c_int, [_P(MdemodRsOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_rs_decode_host": (C.c_int, [_P(MdemodRsOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]),
    "mdemod_rs_vcdu_header": (None, [C.c_void_p, _P(MdemodRsHeader)]),
}
# the host model (csrc/rs_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_rs_model_pn": (None, [C.c_void_p]),
    "mdemod_rs_model_generator": (None, [C.c_void_p]),
    "mdemod_rs_model_dual": (None, [C.c_void_p, C.c_void_p]),
    "mdemod_rs_model_parity": (None, [C.c_void_p, C.c_void_p]),
    "mdemod_rs_model_encode": (C.c_int, [_P(MdemodRsOpts), C.c_void_p, C.c_void_p]),
    "mdemod_rs_model_decode": (C.c_int, [_P(MdemodRsOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


@dataclass
class RsInfo:
    """One frame's verdict: bytes changed in each of the four codewords (255: left as received), and the flags."""
    corrected: tuple
    flags: int

    @property
    def uncorrectable(self) -> bool:
        return bool(self.flags & UNCORRECTABLE)


@dataclass
class Header:
    version: int
    spacecraft: int
    vcid: int
    counter: int


@dataclass
class Report:
    """What ``decode_file`` says about a ``.cadu`` file."""
    frames: int
    uncorrectable_frames: int
    bytes_corrected: int
    frames_per_vcid: dict
    counter_gaps_per_vcid: dict
    list: list


def make_opts(**opts) -> MdemodRsOpts:
    """``mdemod_rs_default_opts`` with the given fields replaced (an unknown name is a TypeError)."""
    o = MdemodRsOpts()
    lib().mdemod_rs_default_opts(C.byref(o))
    names = {f[0] for f in MdemodRsOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"rs: no option {k!r} (there are: {', '.join(sorted(names))})")
        setattr(o, k, int(v))
    return o


def infos(raw) -> list[RsInfo]:
    """uint8 [n, 8] (as the entries write it) to a list of ``RsInfo``."""
    a = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, 8)
    return [RsInfo(tuple(int(x) for x in r[:4]), int(r[4]) | int(r[5]) << 8 | int(r[6]) << 16 | int(r[7]) << 24) for r in a]


def _host_cadu(cadu) -> np.ndarray:
    a = np.ascontiguousarray(cadu, dtype=np.uint8)
    if a.size % CADU_BYTES:
        raise ValueError("CADUs are 1024 bytes each")
    return a.reshape(-1, CADU_BYTES)


def decode(cadu, **opts):
    """CADUs to (VCDUs, report).  A uint8 [n, 1024] device tensor gives device tensors [n, 892] and [n, 8]
    (``mdemod_rs_decode_device``, queued on the current stream; ``infos`` reads the second); a numpy array gives numpy arrays
    (``mdemod_rs_decode_host``, copied in pieces of ``piece_frames``).  Options: the fields of ``mdemod_rs_opts``; ``device`` for a
    numpy array."""
    device = int(opts.pop("device", 0))
    o = make_opts(**opts)
    if isinstance(cadu, np.ndarray):
        a = _host_cadu(cadu)
        n = a.shape[0]
        vcdu, info = np.zeros((n, VCDU_BYTES), dtype=np.uint8), np.zeros((n, 8), dtype=np.uint8)
        check(lib().mdemod_rs_decode_host(C.byref(o), a.ctypes.data, n, vcdu.ctypes.data, info.ctypes.data, device), "mdemod_rs_decode_host")
        return vcdu, info
    import torch
    if not cadu.is_cuda:
        raise ValueError("cadu must be a device tensor or a numpy array")
    if cadu.dtype != torch.uint8 or cadu.dim() != 2 or cadu.shape[1] != CADU_BYTES or not cadu.is_contiguous():
        raise ValueError(f"cadu must be a contiguous uint8 [n, 1024] tensor, got {cadu.dtype} {tuple(cadu.shape)}")
    dev = cadu.device.index or 0
    n = int(cadu.shape[0])
    vcdu = torch.zeros((n, VCDU_BYTES), dtype=torch.uint8, device=cadu.device)
    info = torch.zeros((n, 8), dtype=torch.uint8, device=cadu.device)
    check(lib().mdemod_rs_decode_device(C.byref(o), C.c_void_p(cadu.data_ptr()), n, C.c_void_p(vcdu.data_ptr()), C.c_void_p(info.data_ptr()), dev,
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mdemod_rs_decode_device")
    return vcdu, info


def header(vcdu) -> Header:
    """``mdemod_rs_vcdu_header`` of one VCDU (bytes, or an array)."""
    buf = np.array(np.frombuffer(vcdu, dtype=np.uint8)[:5] if isinstance(vcdu, (bytes, bytearray)) else np.asarray(vcdu, dtype=np.uint8).reshape(-1)[:5])
    if buf.size < 5:
        raise ValueError("a VCDU header needs five bytes")
    h = MdemodRsHeader()
    lib().mdemod_rs_vcdu_header(buf.ctypes.data, C.byref(h))
    return Header(int(h.version), int(h.spacecraft), int(h.vcid), int(h.counter))


def report(vcdu, info) -> Report:
    """Frames, uncorrectable frames, bytes corrected; per VCID (of the frames without an uncorrectable codeword) the frames and the
    places where the 24-bit counter does not follow the VCID's previous frame."""
    lst = infos(info)
    per, gaps, last = {}, {}, {}
    for row, i in zip(np.asarray(vcdu).reshape(-1, VCDU_BYTES), lst):
        if i.uncorrectable:
            continue
        h = header(row)
        per[h.vcid] = per.get(h.vcid, 0) + 1
        gaps.setdefault(h.vcid, 0)
        if h.vcid in last and h.counter != (last[h.vcid] + 1) & 0xFFFFFF:
            gaps[h.vcid] += 1
        last[h.vcid] = h.counter
    fixed = sum(c for i in lst for c in i.corrected if c != FAILED)
    return Report(len(lst), sum(1 for i in lst if i.uncorrectable), fixed, per, gaps, lst)


def decode_file(path, **opts):
    """A ``.cadu`` file to (VCDU bytes, ``Report``)."""
    raw = np.fromfile(str(path), dtype=np.uint8)
    cadu = raw[: raw.size // CADU_BYTES * CADU_BYTES].reshape(-1, CADU_BYTES)
    vcdu, info = decode(cadu, **opts)
    return vcdu.tobytes(), report(vcdu, info)


def soft_to_vcdu(soft, **opts):
    """Soft symbols (int8 [m, 2] device tensor) to (VCDUs [n, 892] device tensor, report [n, 8] device tensor, the frame list):
    ``frames.candidates`` -> ``frames.track`` -> ``frames.viterbi`` -> ``decode``; the symbols, the CADUs and the VCDUs stay on the
    device.  Options: ``min_run`` and ``flywheel`` go to the tracker, ``differential`` and ``skew`` (the link variant of the frame
    layer: Meteor-M N2-3 / N2-4) to all three frame steps, the rest to ``decode``.  ``interleaved`` and ``branch_delay`` (the 80 k
    interleaved mode): the stream is deinterleaved on the device first (``interleave.decode``), and ``skew`` is off after that."""
    from . import frames
    soft = frames._deinterleaved(soft, opts)
    track_opts = {k: opts.pop(k) for k in ("min_run", "flywheel") if k in opts}
    link = {k: opts.pop(k) for k in ("differential", "skew") if k in opts}
    found = frames.track(frames.candidates(soft, **link), int(soft.shape[0]), **link, **track_opts)
    cadu, found = frames.viterbi(soft, found, **link)
    vcdu, info = decode(cadu, **opts)
    return vcdu, info, found


# ------------------------------------------------------------------------------------------------------------- the host model
def pn() -> np.ndarray:
    """One period (255 bytes) of the randomiser's sequence."""
    out = np.zeros(255, dtype=np.uint8)
    lib().mdemod_rs_model_pn(out.ctypes.data)
    return out


def model_generator() -> np.ndarray:
    out = np.zeros(33, dtype=np.uint8)
    lib().mdemod_rs_model_generator(out.ctypes.data)
    return out


def model_dual():
    t, tinv = np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    lib().mdemod_rs_model_dual(t.ctypes.data, tinv.ctypes.data)
    return t, tinv


def model_parity(data) -> np.ndarray:
    a = np.ascontiguousarray(data, dtype=np.uint8)
    if a.size != 223:
        raise ValueError("a codeword has 223 data bytes")
    out = np.zeros(32, dtype=np.uint8)
    lib().mdemod_rs_model_parity(a.ctypes.data, out.ctypes.data)
    return out


def model_encode(vcdu, **opts) -> np.ndarray:
    """892 bytes to one CADU (uint8 [1024]): marker, parity, interleave, and per options dual basis and randomiser."""
    a = np.frombuffer(bytes(vcdu), dtype=np.uint8) if isinstance(vcdu, (bytes, bytearray)) else np.ascontiguousarray(vcdu, dtype=np.uint8).reshape(-1)
    if a.size != VCDU_BYTES:
        raise ValueError("a VCDU has 892 bytes")
    o = make_opts(**opts)
    out = np.zeros(CADU_BYTES, dtype=np.uint8)
    check(lib().mdemod_rs_model_encode(C.byref(o), a.ctypes.data, out.ctypes.data), "mdemod_rs_model_encode")
    return out


def model_decode(cadu, **opts):
    """(uint8 [n, 892], uint8 [n, 8]) of the host model."""
    a = _host_cadu(cadu)
    o = make_opts(**opts)
    n = a.shape[0]
    vcdu, info = np.zeros((n, VCDU_BYTES), dtype=np.uint8), np.zeros((n, 8), dtype=np.uint8)
    check(lib().mdemod_rs_model_decode(C.byref(o), a.ctypes.data, n, vcdu.ctypes.data, info.ctypes.data), "mdemod_rs_model_decode")
    return vcdu, info
