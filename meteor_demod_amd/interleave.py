"""The 80 k interleaved mode: include/meteor_demod_amd_interleave.h over ctypes.

``candidates`` is the search for the interleaver's sync word on the GPU (one candidate per window of 2560 symbols, over all 24
sign, rail and skew conventions), ``track`` the tracker (host only, no GPU), ``deinterleave`` the gather (sync words stripped, the
convention resolved, the 36 branches undone), ``decode`` all three steps (a device tensor of raw soft symbols, or a numpy array,
which is uploaded whole), ``decode_file`` a ``.s`` file to deinterleaved soft symbols plus a report.  What comes out is an ordinary
soft-symbol stream for ``frames`` (plain or ``differential``, ``skew`` off).  ``model_*`` is the host model of
csrc/interleave_host.cpp, the kernels' specification.  This module keeps its own binding table, as ``frames.py`` does.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import check
from .frames import Candidate, MdemodFramesCandidate, _cands_to_c, _check_soft, _host_soft, _stream

BRANCHES, PERIOD_SYMBOLS, WINDOW_SYMBOLS, HYPOTHESES, FULL_SCORE = 36, 40, 2560, 24, 24576


class MdemodIlOpts(C.Structure):
    _fields_ = [("branch_delay", C.c_uint32), ("min_run", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class MdemodIlSegment(C.Structure):
    _fields_ = [("first_symbol", C.c_uint64), ("marker_symbol", C.c_uint64), ("period", C.c_uint64), ("phase", C.c_uint32),
                ("hypothesis", C.c_uint32)]


_P = C.POINTER
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_interleave.h
SIGNATURES = {
    "mdemod_il_default_opts": (None, [_P(MdemodIlOpts)]),
    "mdemod_il_windows": (C.c_uint64, [C.c_uint64]),
    "mdemod_il_max_output_symbols": (C.c_uint64, [C.c_uint64]),
    "mdemod_il_candidates_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_il_track": (C.c_int, [_P(MdemodIlOpts), _P(MdemodFramesCandidate), C.c_uint64, C.c_uint64, _P(MdemodIlSegment), C.c_uint64,
                                  _P(C.c_uint64), _P(C.c_uint64)]),
    "mdemod_il_deinterleave_device": (C.c_int, [_P(MdemodIlOpts), C.c_void_p, C.c_uint64, _P(MdemodIlSegment), C.c_uint64, C.c_uint64, C.c_void_p,
                                                C.c_int, C.c_void_p]),
    "mdemod_il_decode_device": (C.c_int, [_P(MdemodIlOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _P(MdemodIlSegment), C.c_uint64,
                                          _P(C.c_uint64), _P(C.c_uint64), _P(C.c_int32), C.c_int, C.c_void_p]),
    "mdemod_il_decode_host": (C.c_int, [_P(MdemodIlOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _P(MdemodIlSegment), C.c_uint64,
                                        _P(C.c_uint64), _P(C.c_uint64), _P(C.c_int32), C.c_int]),
}
# the host model (csrc/interleave_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_il_model_pattern": (None, [C.c_void_p, C.c_void_p]),
    "mdemod_il_model_candidates": (C.c_int, [C.c_void_p, C.c_uint64, _P(MdemodFramesCandidate)]),
    "mdemod_il_model_deinterleave": (C.c_int, [_P(MdemodIlOpts), C.c_void_p, C.c_uint64, _P(MdemodIlSegment), C.c_uint64, C.c_uint64, C.c_void_p]),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


@dataclass
class Segment:
    """A stretch of the stream with one sync phase and one hypothesis: it begins at ``first_symbol``, its first sync word stands at
    ``marker_symbol`` (x0), which is the sender's period ``period`` (N0)."""
    first_symbol: int
    marker_symbol: int
    period: int
    phase: int
    hypothesis: int


@dataclass
class Report:
    """What ``decode`` and ``decode_file`` say about a pass.  ``mean_score`` is the mean of the windows' sync scores; ``FULL_SCORE``
    is what a clean link at the demodulator's nominal amplitude gives."""
    symbols: int
    segments: int
    periods: int
    mean_score: int
    list: list


def make_opts(**opts) -> MdemodIlOpts:
    """``mdemod_il_default_opts`` with the given fields replaced (an unknown name is a TypeError)."""
    o = MdemodIlOpts()
    lib().mdemod_il_default_opts(C.byref(o))
    names = {f[0] for f in MdemodIlOpts._fields_} - {"reserved"}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"interleave: no option {k!r} (there are: {', '.join(sorted(names))})")
        setattr(o, k, int(v))
    return o


def windows(m: int) -> int:
    return int(lib().mdemod_il_windows(int(m)))


def max_output_symbols(m: int) -> int:
    return int(lib().mdemod_il_max_output_symbols(int(m)))


def _segments(arr, n) -> list[Segment]:
    return [Segment(int(s.first_symbol), int(s.marker_symbol), int(s.period), int(s.phase), int(s.hypothesis)) for s in arr[:n]]


def _segs_to_c(segments: list[Segment]):
    arr = (MdemodIlSegment * max(1, len(segments)))()
    for a, s in zip(arr, segments):
        a.first_symbol, a.marker_symbol, a.period, a.phase, a.hypothesis = s.first_symbol, s.marker_symbol, s.period, s.phase, s.hypothesis
    return arr


def candidates_tensor(soft):
    """``mdemod_il_candidates_device`` as it writes: an int32 [windows, 4] device tensor (position low, position high, score,
    hypothesis), queued on the current stream."""
    import torch
    _check_soft(soft)
    dev = soft.device.index or 0
    m = int(soft.shape[0])
    out = torch.zeros((windows(m), 4), dtype=torch.int32, device=soft.device)
    check(lib().mdemod_il_candidates_device(C.c_void_p(soft.data_ptr()), m, C.c_void_p(out.data_ptr()), dev, _stream(dev)), "mdemod_il_candidates_device")
    return out


def _cands_of(rows) -> list[Candidate]:
    a = np.asarray(rows).astype(np.int64).reshape(-1, 4)
    return [Candidate(int((r[0] & 0xFFFFFFFF) | (r[1] << 32)), int(r[3]), int(r[2])) for r in a]


def candidates(soft) -> list[Candidate]:
    """One candidate per window of ``soft`` (int8 [m, 2] device tensor): position = 2560 w + phase, hypothesis = H, score."""
    return _cands_of(candidates_tensor(soft).cpu().numpy())


def track(cands: list[Candidate], m: int, **opts):
    """``mdemod_il_track`` (no GPU): (the segments, P) of a stream of ``m`` symbols.  Option: ``min_run``."""
    o = make_opts(**opts)
    cap = max(1, len(cands))
    out = (MdemodIlSegment * cap)()
    n, p = C.c_uint64(), C.c_uint64()
    check(lib().mdemod_il_track(C.byref(o), _cands_to_c(cands), len(cands), int(m), out, cap, C.byref(n), C.byref(p)), "mdemod_il_track")
    return _segments(out, min(n.value, cap)), int(p.value)


def deinterleave(soft, segments: list[Segment], n_periods: int, **opts):
    """``mdemod_il_deinterleave_device``: an int8 [36 n_periods, 2] device tensor, queued on the current stream.  Option:
    ``branch_delay``."""
    import torch
    _check_soft(soft)
    o = make_opts(**opts)
    dev = soft.device.index or 0
    out = torch.zeros((BRANCHES * int(n_periods), 2), dtype=torch.int8, device=soft.device)
    check(lib().mdemod_il_deinterleave_device(C.byref(o), C.c_void_p(soft.data_ptr()), int(soft.shape[0]), _segs_to_c(segments), len(segments),
                                              int(n_periods), C.c_void_p(out.data_ptr()), dev, _stream(dev)), "mdemod_il_deinterleave_device")
    return out


def decode(soft, **opts):
    """Sync search, tracker and gather: (the deinterleaved soft symbols, ``Report``).  ``soft`` is an int8 [m, 2] device tensor
    (``mdemod_il_decode_device``: a device tensor comes back) or a numpy array (``mdemod_il_decode_host``: uploaded whole, a numpy
    array comes back).  Options: ``branch_delay``, ``min_run``; ``device`` for a numpy array."""
    device = int(opts.pop("device", 0))
    o = make_opts(**opts)
    n, p, mean = C.c_uint64(), C.c_uint64(), C.c_int32()
    if isinstance(soft, np.ndarray):
        a = _host_soft(soft)
        m = a.shape[0]
        room, cap = max_output_symbols(m), max(1, windows(m))
        segs, out = (MdemodIlSegment * cap)(), np.zeros((room, 2), dtype=np.int8)
        check(lib().mdemod_il_decode_host(C.byref(o), a.ctypes.data, m, out.ctypes.data, room, segs, cap, C.byref(n), C.byref(p), C.byref(mean), device),
              "mdemod_il_decode_host")
        out = out[: min(BRANCHES * p.value, room // BRANCHES * BRANCHES)].copy()
    else:
        import torch
        _check_soft(soft)
        dev = soft.device.index or 0
        m = int(soft.shape[0])
        room, cap = max_output_symbols(m), max(1, windows(m))
        segs, out = (MdemodIlSegment * cap)(), torch.zeros((room, 2), dtype=torch.int8, device=soft.device)
        check(lib().mdemod_il_decode_device(C.byref(o), C.c_void_p(soft.data_ptr()), m, C.c_void_p(out.data_ptr()), room, segs, cap, C.byref(n),
                                            C.byref(p), C.byref(mean), dev, _stream(dev)), "mdemod_il_decode_device")
        out = out[: min(BRANCHES * p.value, room // BRANCHES * BRANCHES)]
    lst = _segments(segs, min(n.value, cap))
    return out, Report(int(m), int(n.value), int(p.value), int(mean.value), lst)


def decode_file(path, **opts):
    """A ``.s`` file of raw soft symbols to (the deinterleaved soft symbols as bytes, ``Report``)."""
    raw = np.fromfile(str(path), dtype=np.int8)
    soft = raw[: raw.size // 2 * 2].reshape(-1, 2)
    out, rep = decode(soft, **opts)
    return out.tobytes(), rep


# ------------------------------------------------------------------------------------------------------------- the host model
def model_pattern():
    a, b = np.zeros(4, dtype=np.int8), np.zeros(4, dtype=np.int8)
    lib().mdemod_il_model_pattern(a.ctypes.data, b.ctypes.data)
    return a, b


def model_candidates(soft) -> list[Candidate]:
    a = _host_soft(soft)
    n = windows(a.shape[0])
    out = (MdemodFramesCandidate * max(1, n))()
    check(lib().mdemod_il_model_candidates(a.ctypes.data, a.shape[0], out), "mdemod_il_model_candidates")
    return [Candidate(int(c.position), int(c.hypothesis), int(c.score)) for c in out[:n]]


def model_deinterleave(soft, segments: list[Segment], n_periods: int, **opts) -> np.ndarray:
    a = _host_soft(soft)
    o = make_opts(**opts)
    out = np.zeros((BRANCHES * int(n_periods), 2), dtype=np.int8)
    check(lib().mdemod_il_model_deinterleave(C.byref(o), a.ctypes.data, a.shape[0], _segs_to_c(segments), len(segments), int(n_periods),
                                             out.ctypes.data), "mdemod_il_model_deinterleave")
    return out


def model_decode(soft, **opts):
    """The model's three steps: (int8 [36 P, 2], the segments, P)."""
    track_opts = {k: opts[k] for k in ("min_run",) if k in opts}
    a = _host_soft(soft)
    segs, p = track(model_candidates(a), a.shape[0], **track_opts)
    return model_deinterleave(a, segs, p, **{k: opts[k] for k in ("branch_delay",) if k in opts}), segs, p
