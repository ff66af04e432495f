"""Survey of a wide recording: include/meteor_demod_amd_survey.h over ctypes.

``spectrum`` is the averaged Hann periodogram of a whole recording on the GPU (rows = a waterfall), ``detect`` the matched
detector on such a spectrum (host only, no GPU), ``survey`` both plus the confirmation of every candidate by the symbol-rate
and 4th-power lines: the hit to hand to ``FrontEndConfig(hit.offset_hz, D)`` is the first one that is ``confirmed``.
This module keeps its own binding table, as ``frontend.py`` does.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import MdemodParams, check
from .demod import DemodConfig

MIN_FFT, MAX_FFT, MAX_ROWS, MAX_CANDIDATES = 256, 16384, 4096, 32


class MdemodSurveyOpts(C.Structure):
    _fields_ = [("fft_size", C.c_uint32), ("n_rows", C.c_uint32), ("max_candidates", C.c_uint32), ("decimation", C.c_int32),
                ("min_snr_db", C.c_double), ("clock_threshold", C.c_float), ("carrier_threshold", C.c_float)]


class MdemodSurveyHit(C.Structure):
    _fields_ = [("offset_hz", C.c_double), ("coarse_offset_hz", C.c_double), ("psd_snr_db", C.c_float), ("clock_quality", C.c_float),
                ("carrier_quality", C.c_float), ("best_row", C.c_uint32), ("confirmed", C.c_int32), ("refined", C.c_int32)]


_P = C.POINTER
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_survey.h
SIGNATURES = {
    "mdemod_survey_default_opts": (None, [_P(MdemodSurveyOpts)]),
    "mdemod_survey_plan": (C.c_int, [_P(MdemodParams), _P(C.c_uint32), _P(C.c_int32)]),
    "mdemod_spectrum_device": (C.c_int, [_P(MdemodParams), C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mdemod_survey_detect": (C.c_int, [_P(MdemodParams), _P(MdemodSurveyOpts), C.c_void_p, C.c_uint32, C.c_uint32, _P(MdemodSurveyHit),
                                       C.c_uint32, _P(C.c_uint32)]),
    "mdemod_survey_device": (C.c_int, [_P(MdemodParams), _P(MdemodSurveyOpts), C.c_void_p, C.c_uint64, _P(MdemodSurveyHit), C.c_uint32,
                                       _P(C.c_uint32), C.c_void_p]),
    "mdemod_survey_host": (C.c_int, [_P(MdemodParams), _P(MdemodSurveyOpts), C.c_void_p, C.c_uint64, _P(MdemodSurveyHit), C.c_uint32,
                                     _P(C.c_uint32)]),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with the survey's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES)


@dataclass
class Hit:
    """One candidate.  ``offset_hz`` is the refined offset when ``refined``, else the coarse one."""
    offset_hz: float
    coarse_offset_hz: float
    psd_snr_db: float
    clock_quality: float
    carrier_quality: float
    best_row: int
    confirmed: bool
    refined: bool


def _hits(arr, n) -> list[Hit]:
    return [Hit(h.offset_hz, h.coarse_offset_hz, h.psd_snr_db, h.clock_quality, h.carrier_quality, int(h.best_row), bool(h.confirmed),
                bool(h.refined)) for h in arr[:n]]


def make_opts(**opts) -> MdemodSurveyOpts:
    """``mdemod_survey_default_opts`` with the given fields replaced (an unknown name is a TypeError)."""
    o = MdemodSurveyOpts()
    lib().mdemod_survey_default_opts(C.byref(o))
    names = {f[0] for f in MdemodSurveyOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"survey: no option {k!r} (there are: {', '.join(sorted(names))})")
        setattr(o, k, v)
    return o


def survey_plan(cfg: DemodConfig) -> tuple[int, int]:
    """``mdemod_survey_plan`` (CPU only): (default fft_size, the largest decimation the front end accepts)."""
    p = cfg.to_c(1)
    n, d = C.c_uint32(), C.c_int32()
    check(lib().mdemod_survey_plan(C.byref(p), C.byref(n), C.byref(d)), "mdemod_survey_plan")
    return int(n.value), int(d.value)


def _check_iq(cfg: DemodConfig, iq):
    import torch
    want = {8: torch.uint8, 16: torch.int16, 32: torch.float32}.get(cfg.bps)
    if not iq.is_cuda:
        raise ValueError("iq must be a device tensor")
    if iq.dtype != want:
        raise ValueError(f"iq dtype {iq.dtype} does not match bps={cfg.bps} ({want})")
    if iq.dim() != 2 or iq.shape[1] != 2 or not iq.is_contiguous():
        raise ValueError(f"iq must be a contiguous [n, 2] tensor, got {tuple(iq.shape)}")


def spectrum(cfg: DemodConfig, iq, fft_size: int | None = None, rows: int = 1):
    """``mdemod_spectrum_device``: float32 [rows, fft_size] device tensor, row r the mean Hann periodogram of the r-th run of
    segments of ``iq`` ([n, 2] device tensor in the format of ``cfg.bps``), bin 0 = -fs / 2."""
    import torch
    _check_iq(cfg, iq)
    n_fft = int(fft_size) if fft_size else survey_plan(cfg)[0]
    dev = iq.device.index or 0
    p = cfg.to_c(1, dev)
    if not (MIN_FFT <= n_fft <= MAX_FFT) or not (1 <= int(rows) <= MAX_ROWS):
        psd = torch.empty((1,), dtype=torch.float32, device=iq.device)      # (the library refuses, with its own words)
    else:
        psd = torch.empty((int(rows), n_fft), dtype=torch.float32, device=iq.device)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mdemod_spectrum_device(C.byref(p), C.c_void_p(iq.data_ptr()), int(iq.shape[0]), n_fft, int(rows), C.c_void_p(psd.data_ptr()), st),
          "mdemod_spectrum_device")
    return psd


def detect(cfg: DemodConfig, psd, **opts) -> list[Hit]:
    """``mdemod_survey_detect`` (no GPU): the candidates in ``psd`` ([rows, fft_size] or [fft_size]; numpy, or a tensor, which is
    fetched), strongest first.  Options: ``max_candidates``, ``min_snr_db``."""
    if hasattr(psd, "detach"):
        psd = psd.detach().cpu().numpy()
    a = np.ascontiguousarray(psd, dtype=np.float32)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2:
        raise ValueError(f"psd must be [rows, fft_size], got {a.shape}")
    o = make_opts(**opts)
    p = cfg.to_c(1)
    out = (MdemodSurveyHit * MAX_CANDIDATES)()
    n = C.c_uint32()
    check(lib().mdemod_survey_detect(C.byref(p), C.byref(o), a.ctypes.data, a.shape[1], a.shape[0], out, MAX_CANDIDATES, C.byref(n)),
          "mdemod_survey_detect")
    return _hits(out, min(n.value, MAX_CANDIDATES))


def survey(cfg: DemodConfig, iq, **opts) -> list[Hit]:
    """``mdemod_survey_device`` (a device tensor [n, 2]) or ``mdemod_survey_host`` (a numpy array [n, 2]): confirmed hits first,
    then by ``psd_snr_db``.  Options: the fields of ``mdemod_survey_opts``."""
    o = make_opts(**opts)
    out = (MdemodSurveyHit * MAX_CANDIDATES)()
    n = C.c_uint32()
    if isinstance(iq, np.ndarray):
        dt = {8: np.uint8, 16: np.int16, 32: np.float32}[cfg.bps]
        a = np.ascontiguousarray(iq, dtype=dt).reshape(-1, 2)
        p = cfg.to_c(1)
        check(lib().mdemod_survey_host(C.byref(p), C.byref(o), a.ctypes.data, a.shape[0], out, MAX_CANDIDATES, C.byref(n)), "mdemod_survey_host")
    else:
        import torch
        _check_iq(cfg, iq)
        dev = iq.device.index or 0
        p = cfg.to_c(1, dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib().mdemod_survey_device(C.byref(p), C.byref(o), C.c_void_p(iq.data_ptr()), int(iq.shape[0]), out, MAX_CANDIDATES, C.byref(n), st),
              "mdemod_survey_device")
    return _hits(out, min(n.value, MAX_CANDIDATES))
