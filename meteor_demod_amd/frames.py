"""The frame layer: include/meteor_demod_amd_frames.h over ctypes.

``candidates`` is the marker search on the GPU (one candidate per window of 8192 symbols), ``track`` the tracker (host only, no
GPU), ``decode`` all three steps (a device tensor of soft symbols, or a numpy array, which is copied in pieces), ``decode_file``
a ``.s`` file to CADU bytes plus a report.  ``model_*`` is the host model of csrc/frames_host.cpp, the kernels' specification.
This module keeps its own binding table, as ``survey.py`` does.

The link variant (include/meteor_demod_amd_frames_link.h: Meteor-M N2-3 / N2-4) is chosen by two keywords on ``candidates``,
``track``, ``viterbi``, ``decode``, ``decode_file`` and ``model_*``: ``differential=True`` for an NRZ-M coded sender, ``skew=True``
to let the rails stand one symbol apart (OQPSK).  ``hypothesis`` then carries H = h + 8 s.  With both off (the default) the plain
entries are called.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import check

FRAME_SYMBOLS, FRAME_BYTES, FRAME_DECISIONS, FLYWHEEL = 8192, 1024, 16372, 1


class MdemodFramesOpts(C.Structure):
    _fields_ = [("min_run", C.c_uint32), ("flywheel", C.c_uint32), ("piece_symbols", C.c_uint64)]


class MdemodFramesCandidate(C.Structure):
    _fields_ = [("position", C.c_uint64), ("score", C.c_int32), ("hypothesis", C.c_uint32)]


class MdemodFrameInfo(C.Structure):
    _fields_ = [("position", C.c_uint64), ("score", C.c_int32), ("hypothesis", C.c_uint32), ("flags", C.c_uint32),
                ("channel_errors", C.c_uint32), ("run", C.c_uint32), ("reserved", C.c_uint32)]


class MdemodFramesLink(C.Structure):
    _fields_ = [("differential", C.c_uint32), ("skew", C.c_uint32), ("reserved", C.c_uint32 * 2)]


_P = C.POINTER
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_frames.h
SIGNATURES = {
    "mdemod_frames_default_opts": (None, [_P(MdemodFramesOpts)]),
    "mdemod_frames_windows": (C.c_uint64, [C.c_uint64]),
    "mdemod_frames_candidates_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_frames_track": (C.c_int, [_P(MdemodFramesOpts), _P(MdemodFramesCandidate), C.c_uint64, C.c_uint64, _P(MdemodFrameInfo), C.c_uint64,
                                      _P(C.c_uint64)]),
    "mdemod_frames_viterbi_device": (C.c_int, [C.c_void_p, C.c_uint64, _P(MdemodFrameInfo), C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_frames_decode_device": (C.c_int, [_P(MdemodFramesOpts), C.c_void_p, C.c_uint64, C.c_void_p, _P(MdemodFrameInfo), C.c_uint64,
                                              _P(C.c_uint64), C.c_int, C.c_void_p]),
    "mdemod_frames_decode_host": (C.c_int, [_P(MdemodFramesOpts), C.c_void_p, C.c_uint64, C.c_void_p, _P(MdemodFrameInfo), C.c_uint64,
                                            _P(C.c_uint64), C.c_int]),
}
# the host model (csrc/frames_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_frames_model_encode": (C.c_uint32, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mdemod_frames_model_pattern": (None, [C.c_void_p, C.c_void_p]),
    "mdemod_frames_model_candidates": (C.c_int, [C.c_void_p, C.c_uint64, _P(MdemodFramesCandidate)]),
    "mdemod_frames_model_viterbi": (C.c_int, [C.c_void_p, C.c_uint64, _P(MdemodFrameInfo), C.c_uint64, C.c_void_p]),
    "mdemod_frames_model_decode": (C.c_int, [_P(MdemodFramesOpts), C.c_void_p, C.c_uint64, C.c_void_p, _P(MdemodFrameInfo), C.c_uint64,
                                             _P(C.c_uint64)]),
}

# every entry of include/meteor_demod_amd_frames_link.h
LINK_SIGNATURES = {
    "mdemod_frames_link_windows": (C.c_uint64, [_P(MdemodFramesLink), C.c_uint64]),
    "mdemod_frames_link_candidates_device": (C.c_int, [_P(MdemodFramesLink), C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_frames_link_track": (C.c_int, [_P(MdemodFramesLink), _P(MdemodFramesOpts), _P(MdemodFramesCandidate), C.c_uint64, C.c_uint64,
                                           _P(MdemodFrameInfo), C.c_uint64, _P(C.c_uint64)]),
    "mdemod_frames_link_viterbi_device": (C.c_int, [_P(MdemodFramesLink), C.c_void_p, C.c_uint64, _P(MdemodFrameInfo), C.c_uint64, C.c_void_p, C.c_int,
                                                    C.c_void_p]),
    "mdemod_frames_link_decode_device": (C.c_int, [_P(MdemodFramesLink), _P(MdemodFramesOpts), C.c_void_p, C.c_uint64, C.c_void_p, _P(MdemodFrameInfo),
                                                   C.c_uint64, _P(C.c_uint64), C.c_int, C.c_void_p]),
    "mdemod_frames_link_decode_host": (C.c_int, [_P(MdemodFramesLink), _P(MdemodFramesOpts), C.c_void_p, C.c_uint64, C.c_void_p, _P(MdemodFrameInfo),
                                                 C.c_uint64, _P(C.c_uint64), C.c_int]),
}
LINK_MODEL_SIGNATURES = {
    "mdemod_frames_model_link_pattern": (None, [_P(MdemodFramesLink), C.c_void_p, C.c_void_p]),
    "mdemod_frames_model_link_candidates": (C.c_int, [_P(MdemodFramesLink), C.c_void_p, C.c_uint64, _P(MdemodFramesCandidate)]),
    "mdemod_frames_model_link_viterbi": (C.c_int, [_P(MdemodFramesLink), C.c_void_p, C.c_uint64, _P(MdemodFrameInfo), C.c_uint64, C.c_void_p]),
    "mdemod_frames_model_link_decode": (C.c_int, [_P(MdemodFramesLink), _P(MdemodFramesOpts), C.c_void_p, C.c_uint64, C.c_void_p, _P(MdemodFrameInfo),
                                                  C.c_uint64, _P(C.c_uint64)]),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with the frame layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES, LINK_SIGNATURES, LINK_MODEL_SIGNATURES)


@dataclass
class Candidate:
    """The best (position, hypothesis) of one window of 8192 positions."""
    position: int
    hypothesis: int
    score: int


@dataclass
class Frame:
    """One frame of 8192 symbols.  ``channel_errors`` (of 16372 hard decisions) is 0 until the frame is decoded."""
    position: int
    hypothesis: int
    score: int
    flags: int
    channel_errors: int
    run: int

    @property
    def flywheel(self) -> bool:
        return bool(self.flags & FLYWHEEL)


@dataclass
class Report:
    """What ``decode_file`` says about a pass."""
    symbols: int
    frames: int
    flywheel_frames: int
    runs: int
    mean_channel_error_rate: float
    list: list


def make_opts(**opts) -> MdemodFramesOpts:
    """``mdemod_frames_default_opts`` with the given fields replaced (an unknown name is a TypeError)."""
    o = MdemodFramesOpts()
    lib().mdemod_frames_default_opts(C.byref(o))
    names = {f[0] for f in MdemodFramesOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"frames: no option {k!r} (there are: {', '.join(sorted(names))})")
        setattr(o, k, v)
    return o


def make_link(differential=False, skew=False):
    """The ``mdemod_frames_link`` of the two keywords, or None when both are off (the plain entries are called then)."""
    for name, v in (("differential", differential), ("skew", skew)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError(f"frames: {name} is a switch (True or False), got {v!r}")
    if not differential and not skew:
        return None
    link = MdemodFramesLink()
    link.differential, link.skew = int(differential), int(skew)
    return link


def windows(m: int, *, skew=False) -> int:
    link = make_link(False, skew)
    return int(lib().mdemod_frames_link_windows(C.byref(link), int(m)) if link else lib().mdemod_frames_windows(int(m)))


def _frames(arr, n) -> list[Frame]:
    return [Frame(int(f.position), int(f.hypothesis), int(f.score), int(f.flags), int(f.channel_errors), int(f.run)) for f in arr[:n]]


def _to_c(frames: list[Frame]):
    arr = (MdemodFrameInfo * max(1, len(frames)))()
    for a, f in zip(arr, frames):
        a.position, a.hypothesis, a.score, a.flags, a.channel_errors, a.run = f.position, f.hypothesis, f.score, f.flags, f.channel_errors, f.run
    return arr


def _cands_to_c(cands: list[Candidate]):
    arr = (MdemodFramesCandidate * max(1, len(cands)))()
    for a, c in zip(arr, cands):
        a.position, a.hypothesis, a.score = c.position, c.hypothesis, c.score
    return arr


def _host_soft(soft) -> np.ndarray:
    a = np.ascontiguousarray(soft, dtype=np.int8)
    if a.size % 2:
        raise ValueError("soft symbols come in (I, Q) pairs")
    return a.reshape(-1, 2)


def _check_soft(soft):
    import torch
    if not soft.is_cuda:
        raise ValueError("soft must be a device tensor")
    if soft.dtype != torch.int8 or soft.dim() != 2 or soft.shape[1] != 2 or not soft.is_contiguous():
        raise ValueError(f"soft must be a contiguous int8 [m, 2] tensor, got {soft.dtype} {tuple(soft.shape)}")


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def candidates_tensor(soft, *, differential=False, skew=False):
    """``mdemod_frames_candidates_device`` (``mdemod_frames_link_candidates_device`` with a switch on) as it writes: an int32
    [windows, 4] device tensor (position low, position high, score, hypothesis), queued on the current stream."""
    import torch
    link = make_link(differential, skew)
    _check_soft(soft)
    dev = soft.device.index or 0
    m = int(soft.shape[0])
    out = torch.zeros((windows(m, skew=skew), 4), dtype=torch.int32, device=soft.device)
    if link is None:
        check(lib().mdemod_frames_candidates_device(C.c_void_p(soft.data_ptr()), m, C.c_void_p(out.data_ptr()), dev, _stream(dev)),
              "mdemod_frames_candidates_device")
    else:
        check(lib().mdemod_frames_link_candidates_device(C.byref(link), C.c_void_p(soft.data_ptr()), m, C.c_void_p(out.data_ptr()), dev, _stream(dev)),
              "mdemod_frames_link_candidates_device")
    return out


def candidates(soft, *, differential=False, skew=False) -> list[Candidate]:
    """One candidate per window of ``soft`` (int8 [m, 2] device tensor)."""
    a = candidates_tensor(soft, differential=differential, skew=skew).cpu().numpy().astype(np.int64)
    return [Candidate(int((r[0] & 0xFFFFFFFF) | (r[1] << 32)), int(r[3]), int(r[2])) for r in a]


def track(cands: list[Candidate], m: int, *, differential=False, skew=False, **opts) -> list[Frame]:
    """``mdemod_frames_track`` (no GPU): the frame list of a stream of ``m`` symbols.  Options: ``min_run``, ``flywheel``."""
    link = make_link(differential, skew)
    o = make_opts(**opts)
    cap = max(1, int(m) // FRAME_SYMBOLS)
    out = (MdemodFrameInfo * cap)()
    n = C.c_uint64()
    if link is None:
        check(lib().mdemod_frames_track(C.byref(o), _cands_to_c(cands), len(cands), int(m), out, cap, C.byref(n)), "mdemod_frames_track")
    else:
        check(lib().mdemod_frames_link_track(C.byref(link), C.byref(o), _cands_to_c(cands), len(cands), int(m), out, cap, C.byref(n)),
              "mdemod_frames_link_track")
    return _frames(out, min(n.value, cap))


def viterbi(soft, frames: list[Frame], *, differential=False, skew=False):
    """``mdemod_frames_viterbi_device``: (uint8 [n, 1024] device tensor, the frames with ``channel_errors``)."""
    import torch
    link = make_link(differential, skew)
    _check_soft(soft)
    dev = soft.device.index or 0
    arr = _to_c(frames)
    out = torch.zeros((len(frames), FRAME_BYTES), dtype=torch.uint8, device=soft.device)
    if link is None:
        check(lib().mdemod_frames_viterbi_device(C.c_void_p(soft.data_ptr()), int(soft.shape[0]), arr, len(frames), C.c_void_p(out.data_ptr()), dev,
                                                 _stream(dev)), "mdemod_frames_viterbi_device")
    else:
        check(lib().mdemod_frames_link_viterbi_device(C.byref(link), C.c_void_p(soft.data_ptr()), int(soft.shape[0]), arr, len(frames),
                                                      C.c_void_p(out.data_ptr()), dev, _stream(dev)), "mdemod_frames_link_viterbi_device")
    return out, _frames(arr, len(frames))


def _deinterleaved(soft, opts: dict, device: int = 0):
    """Takes ``interleaved`` and ``branch_delay`` out of ``opts``.  With ``interleaved`` the stream goes through
    ``interleave.decode`` on the device first and ``skew`` is switched off (the interleaver's sync word has resolved it); without,
    ``soft`` comes back as it is."""
    interleaved, branch_delay = opts.pop("interleaved", False), opts.pop("branch_delay", 2048)
    if not isinstance(interleaved, (bool, np.bool_)):
        raise TypeError(f"frames: interleaved is a switch (True or False), got {interleaved!r}")
    if not interleaved:
        return soft
    from . import interleave
    opts["skew"] = False
    kw = dict(device=device) if isinstance(soft, np.ndarray) else {}
    return interleave.decode(soft, branch_delay=branch_delay, **kw)[0]


def decode(soft, **opts):
    """Sync search, tracker and Viterbi: (uint8 [n, 1024] numpy array of CADUs, list of ``Frame``).  ``soft`` is an int8 [m, 2]
    device tensor (``mdemod_frames_decode_device``) or a numpy array (``mdemod_frames_decode_host``, copied in pieces of
    ``piece_symbols``).  Options: the fields of ``mdemod_frames_opts``; ``device`` for a numpy array; ``differential`` and ``skew``
    (the link variant: ``mdemod_frames_link_decode_*``); ``interleaved`` and ``branch_delay`` (the 80 k interleaved mode: the stream
    is deinterleaved on the device first, ``interleave.decode``, and the frame pass runs with ``skew`` off)."""
    device = int(opts.pop("device", 0))
    soft = _deinterleaved(soft, opts, device)
    link = make_link(opts.pop("differential", False), opts.pop("skew", False))
    o = make_opts(**opts)
    n = C.c_uint64()
    if isinstance(soft, np.ndarray):
        a = _host_soft(soft)
        cap = max(1, a.shape[0] // FRAME_SYMBOLS)
        out, cadu = (MdemodFrameInfo * cap)(), np.zeros((cap, FRAME_BYTES), dtype=np.uint8)
        if link is None:
            check(lib().mdemod_frames_decode_host(C.byref(o), a.ctypes.data, a.shape[0], cadu.ctypes.data, out, cap, C.byref(n), device),
                  "mdemod_frames_decode_host")
        else:
            check(lib().mdemod_frames_link_decode_host(C.byref(link), C.byref(o), a.ctypes.data, a.shape[0], cadu.ctypes.data, out, cap, C.byref(n),
                                                       device), "mdemod_frames_link_decode_host")
    else:
        _check_soft(soft)
        dev = soft.device.index or 0
        cap = max(1, int(soft.shape[0]) // FRAME_SYMBOLS)
        out, cadu = (MdemodFrameInfo * cap)(), np.zeros((cap, FRAME_BYTES), dtype=np.uint8)
        if link is None:
            check(lib().mdemod_frames_decode_device(C.byref(o), C.c_void_p(soft.data_ptr()), int(soft.shape[0]), cadu.ctypes.data, out, cap,
                                                    C.byref(n), dev, _stream(dev)), "mdemod_frames_decode_device")
        else:
            check(lib().mdemod_frames_link_decode_device(C.byref(link), C.byref(o), C.c_void_p(soft.data_ptr()), int(soft.shape[0]), cadu.ctypes.data,
                                                         out, cap, C.byref(n), dev, _stream(dev)), "mdemod_frames_link_decode_device")
    k = min(n.value, cap)
    return cadu[:k].copy(), _frames(out, k)


def report(frames: list[Frame], m: int) -> Report:
    fly = sum(1 for f in frames if f.flywheel)
    rate = float(np.mean([f.channel_errors / FRAME_DECISIONS for f in frames])) if frames else 0.0
    return Report(int(m), len(frames), fly, len({f.run for f in frames}), rate, frames)


def decode_file(path, **opts):
    """A ``.s`` file of soft symbols to (CADU bytes, ``Report``)."""
    raw = np.fromfile(str(path), dtype=np.int8)
    soft = raw[: raw.size // 2 * 2].reshape(-1, 2)
    cadu, frames = decode(soft, **opts)
    return cadu.tobytes(), report(frames, soft.shape[0])


# ------------------------------------------------------------------------------------------------------------- the host model
def model_encode(data: bytes, reg: int = 0):
    """(int8 [8 n, 2] of +-1, the register after): ``data`` through the encoder from register ``reg``."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    sym = np.zeros((8 * buf.size, 2), dtype=np.int8)
    reg = lib().mdemod_frames_model_encode(buf.ctypes.data, buf.size, reg, sym.ctypes.data)
    return sym, int(reg)


def model_pattern(*, differential=False):
    a, b = np.zeros(26, dtype=np.int8), np.zeros(26, dtype=np.int8)
    link = make_link(differential, False)
    if link is None:
        lib().mdemod_frames_model_pattern(a.ctypes.data, b.ctypes.data)
    else:
        lib().mdemod_frames_model_link_pattern(C.byref(link), a.ctypes.data, b.ctypes.data)
    return a, b


def model_candidates(soft, *, differential=False, skew=False) -> list[Candidate]:
    link = make_link(differential, skew)
    a = _host_soft(soft)
    n = windows(a.shape[0], skew=skew)
    out = (MdemodFramesCandidate * max(1, n))()
    if link is None:
        check(lib().mdemod_frames_model_candidates(a.ctypes.data, a.shape[0], out), "mdemod_frames_model_candidates")
    else:
        check(lib().mdemod_frames_model_link_candidates(C.byref(link), a.ctypes.data, a.shape[0], out), "mdemod_frames_model_link_candidates")
    return [Candidate(int(c.position), int(c.hypothesis), int(c.score)) for c in out[:n]]


def model_viterbi(soft, frames: list[Frame], *, differential=False, skew=False):
    link = make_link(differential, skew)
    a = _host_soft(soft)
    arr = _to_c(frames)
    cadu = np.zeros((len(frames), FRAME_BYTES), dtype=np.uint8)
    if link is None:
        check(lib().mdemod_frames_model_viterbi(a.ctypes.data, a.shape[0], arr, len(frames), cadu.ctypes.data), "mdemod_frames_model_viterbi")
    else:
        check(lib().mdemod_frames_model_link_viterbi(C.byref(link), a.ctypes.data, a.shape[0], arr, len(frames), cadu.ctypes.data),
              "mdemod_frames_model_link_viterbi")
    return cadu, _frames(arr, len(frames))


def model_decode(soft, **opts):
    link = make_link(opts.pop("differential", False), opts.pop("skew", False))
    a = _host_soft(soft)
    o = make_opts(**opts)
    cap = max(1, a.shape[0] // FRAME_SYMBOLS)
    out, cadu = (MdemodFrameInfo * cap)(), np.zeros((cap, FRAME_BYTES), dtype=np.uint8)
    n = C.c_uint64()
    if link is None:
        check(lib().mdemod_frames_model_decode(C.byref(o), a.ctypes.data, a.shape[0], cadu.ctypes.data, out, cap, C.byref(n)), "mdemod_frames_model_decode")
    else:
        check(lib().mdemod_frames_model_link_decode(C.byref(link), C.byref(o), a.ctypes.data, a.shape[0], cadu.ctypes.data, out, cap, C.byref(n)),
              "mdemod_frames_model_link_decode")
    k = min(n.value, cap)
    return cadu[:k].copy(), _frames(out, k)
