"""Front end (digital down-converter) ahead of the demodulator: include/meteor_demod_amd_frontend.h over ctypes.

A signal ``offset_hz`` from the recording's centre is moved to 0 Hz, low-pass filtered and decimated by ``decimation`` on the
GPU; the demodulator then runs on that f32 baseband at ``samplerate / decimation`` exactly as on any f32 recording.  The
baseband is this library's own arithmetic (a pure function of input, absolute index and settings); the demodulator on it is
the reference's, bit for bit.  This module keeps its own binding table: the main header's (``_capi.SIGNATURES``) stays as it is.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass, replace

import numpy as np

from . import _capi
from ._capi import MdemodLockEvent, MdemodParams, MdemodRecordingReport, MdemodStatus, check
from .demod import DemodConfig

DEFAULT_TAPS_PER_PHASE = 16
MAX_TAPS = 32 * 128 + 1


class MdemodFeParams(C.Structure):
    _fields_ = [("offset_hz", C.c_double), ("decimation", C.c_int32), ("taps_per_phase", C.c_int32),
                ("offsets_hz", C.POINTER(C.c_double))]


_P = C.POINTER
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_frontend.h
SIGNATURES = {
    "mdemod_fe_design": (C.c_int, [_P(MdemodParams), _P(MdemodFeParams), _P(C.c_float), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "mdemod_fe_create": (C.c_int, [_P(MdemodParams), _P(MdemodFeParams), _P(C.c_void_p)]),
    "mdemod_fe_destroy": (None, [C.c_void_p]),
    "mdemod_fe_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mdemod_fe_demodulator": (C.c_void_p, [C.c_void_p]),
    "mdemod_fe_max_outputs": (C.c_uint64, [C.c_void_p, C.c_uint64]),
    "mdemod_fe_baseband_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                            C.c_void_p, C.c_void_p]),
    "mdemod_fe_process_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                           C.c_uint32, C.c_void_p]),
    "mdemod_fe_process_host": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_uint32), _P(C.c_void_p), _P(C.c_uint32),
                                         _P(C.c_uint32)]),
    "mdemod_fe_demodulate_recording_host": (C.c_int, [_P(MdemodParams), _P(MdemodFeParams), _P(_capi.MdemodRecordingOpts), C.c_void_p,
                                                      C.c_uint64, C.c_void_p, C.c_uint64, _P(MdemodRecordingReport)]),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with the front end's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES)


@dataclass
class FrontEndConfig:
    """Where the signal sits in the recording and how much to decimate.  ``offset_hz`` is moved to 0 Hz."""
    offset_hz: float
    decimation: int
    taps_per_phase: int = DEFAULT_TAPS_PER_PHASE

    def to_c(self, offsets=None):
        arr = None
        if offsets is not None:
            arr = (C.c_double * len(offsets))(*[float(o) for o in offsets])
        p = MdemodFeParams(float(self.offset_hz), int(self.decimation), int(self.taps_per_phase),
                           C.cast(arr, C.POINTER(C.c_double)) if arr is not None else None)
        return p, arr                                     # (arr keeps the offsets alive as long as the caller holds it)


def output_config(cfg: DemodConfig, fe: FrontEndConfig) -> DemodConfig:
    """The demodulator's settings behind the front end: samplerate / D, f32 input."""
    return replace(cfg, samplerate=cfg.samplerate // int(fe.decimation), bps=32)


def phase_step(offset_hz: float, samplerate: int) -> int:
    """llround(-offset / fs * 2^32) mod 2^32 (C's llround: halves away from zero)."""
    v = -offset_hz / samplerate * 4294967296.0
    r = math.floor(abs(v) + 0.5)
    return int(math.copysign(r, v)) & 0xFFFFFFFF


def design_taps(cfg: DemodConfig, fe: FrontEndConfig, n_streams: int = 1, offsets=None):
    """``mdemod_fe_design`` (CPU only): (taps float32 [L], phase step of the first stream)."""
    L = lib()
    p = cfg.to_c(n_streams)
    fp, _keep = fe.to_c(offsets)
    taps = np.zeros(MAX_TAPS, dtype=np.float32)
    n = C.c_uint32()
    step = C.c_uint32()
    check(L.mdemod_fe_design(C.byref(p), C.byref(fp), taps.ctypes.data_as(C.POINTER(C.c_float)), MAX_TAPS, C.byref(n), C.byref(step)),
          "mdemod_fe_design")
    return taps[: n.value].copy(), int(step.value)


class FrontEnd:
    """Front end + demodulator for ``n_streams`` streams of the INPUT described by ``cfg`` (samplerate, bps of the recording).
    ``offsets``: one offset per stream (several channels of one recording), else ``fe.offset_hz`` for all."""

    def __init__(self, cfg: DemodConfig, fe: FrontEndConfig, n_streams: int = 1, offsets=None, device: int = 0):
        self.cfg = cfg
        self.fe = fe
        self.out_cfg = output_config(cfg, fe)
        self.n_streams = int(n_streams)
        self.device = int(device)
        self._lib = lib()
        self._h = C.c_void_p()
        p = cfg.to_c(n_streams, device)
        fp, keep = fe.to_c(offsets)
        if offsets is not None and len(offsets) != self.n_streams:
            raise ValueError(f"{len(offsets)} offsets for {self.n_streams} streams")
        check(self._lib.mdemod_fe_create(C.byref(p), C.byref(fp), C.byref(self._h)), "mdemod_fe_create")
        del keep
        self._ctx = C.c_void_p(self._lib.mdemod_fe_demodulator(self._h))

    # -- lifecycle -----------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.mdemod_fe_destroy(self._h)
            self._h = C.c_void_p()
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self) -> None:
        check(self._lib.mdemod_fe_reset(self._h, self._stream()), "mdemod_fe_reset")

    # -- helpers ---------------------------------------------------------------
    def _stream(self) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def max_outputs(self, n_samples: int) -> int:
        return int(self._lib.mdemod_fe_max_outputs(self._h, int(n_samples)))

    def _check_iq(self, iq) -> None:
        import torch
        want = {8: torch.uint8, 16: torch.int16, 32: torch.float32}[self.cfg.bps]
        if not iq.is_cuda or iq.device.index != self.device:
            raise ValueError(f"iq lives on {iq.device}, this front end on cuda:{self.device}")
        if iq.dtype != want:
            raise ValueError(f"iq dtype {iq.dtype} does not match bps={self.cfg.bps} ({want})")

    def _uniform_rows(self, iq):
        import torch
        self._check_iq(iq)
        if iq.dim() != 3 or iq.shape[0] != self.n_streams or iq.shape[2] != 2 or iq.stride(2) != 1 or iq.stride(1) != 2:
            raise ValueError(f"iq must be [n_streams={self.n_streams}, n, 2] with contiguous samples, got {tuple(iq.shape)}")
        n = int(iq.shape[1])
        off = torch.arange(self.n_streams, dtype=torch.int64, device=iq.device) * (iq.stride(0) // 2)
        cnt = torch.full((self.n_streams,), n, dtype=torch.int32, device=iq.device)
        return n, off, cnt

    @staticmethod
    def _iq_ptr(iq_flat) -> C.c_void_p:
        """An empty batch has no storage (data_ptr 0), and the library refuses a NULL input: any valid address will do there."""
        if iq_flat.numel() == 0:
            import torch
            return C.c_void_p(torch.zeros(16, dtype=torch.uint8, device=iq_flat.device).data_ptr())
        return C.c_void_p(iq_flat.data_ptr())

    def _check_ragged(self, iq_flat, offsets, counts) -> None:
        self._check_iq(iq_flat)
        if iq_flat.dim() != 2 or iq_flat.shape[1] != 2 or not iq_flat.is_contiguous():
            raise ValueError("iq_flat must be a contiguous [total, 2] tensor")
        for name, t, size in (("offsets", offsets, 8), ("counts", counts, 4)):
            if (t.device != iq_flat.device or t.numel() != self.n_streams or t.element_size() != size or not t.is_contiguous()
                    or t.is_floating_point()):
                raise ValueError(f"{name} must be a contiguous {size * 8}-bit integer tensor of {self.n_streams} entries on {iq_flat.device}")

    # -- front end only --------------------------------------------------------
    def baseband_ragged(self, iq_flat, offsets, counts, max_samples: int):
        """``mdemod_fe_baseband_device``: (bb float32 [n_streams, cap, 2] device tensor, n_out int32 device tensor).
        Every count must be <= ``max_samples``; ``iq_flat`` [total, 2], offsets int64, counts int32 (device)."""
        import torch
        self._check_ragged(iq_flat, offsets, counts)
        cap = max(self.max_outputs(max_samples), 1)
        bb = torch.empty((self.n_streams, cap, 2), dtype=torch.float32, device=iq_flat.device)
        n_out = torch.zeros((self.n_streams,), dtype=torch.int32, device=iq_flat.device)
        check(self._lib.mdemod_fe_baseband_device(self._h, self._iq_ptr(iq_flat), C.c_void_p(offsets.data_ptr()),
                                                  C.c_void_p(counts.data_ptr()), C.c_void_p(bb.data_ptr()), cap, cap,
                                                  C.c_void_p(n_out.data_ptr()), self._stream()), "mdemod_fe_baseband_device")
        return bb, n_out

    def baseband(self, iq):
        """Front end on one block per stream (``iq`` [n_streams, n, 2] device tensor in the input's format): returns
        (bb float32 [n_streams, cap, 2] device tensor, numpy array of the per-stream output counts) - synchronises."""
        import torch
        n, off, cnt = self._uniform_rows(iq)
        base = iq.as_strided(((self.n_streams - 1) * (iq.stride(0) // 2) + n, 2), (2, 1))
        bb, n_out = self.baseband_ragged(base, off, cnt, n)
        torch.cuda.synchronize(self.device)
        return bb, n_out.cpu().numpy().astype(np.int64)

    # -- front end + demodulator -----------------------------------------------
    def max_symbols(self, n_samples: int) -> int:
        return self.max_outputs(n_samples) + 8

    def process_ragged(self, iq_flat, offsets, counts, max_samples: int, soft=None):
        """``mdemod_fe_process_device`` on a ragged batch; ``soft`` int8 [n_streams, cap, 2] (made when None)."""
        import torch
        self._check_ragged(iq_flat, offsets, counts)
        cap = self.max_symbols(max_samples)
        if soft is None:
            soft = torch.empty((self.n_streams, cap, 2), dtype=torch.int8, device=iq_flat.device)
        if (not soft.is_cuda or soft.dtype != torch.int8 or soft.dim() != 3 or soft.shape[0] != self.n_streams or soft.shape[2] != 2
                or not soft.is_contiguous()):
            raise ValueError(f"soft must be a contiguous int8 [n_streams={self.n_streams}, cap, 2] tensor")
        check(self._lib.mdemod_fe_process_device(self._h, self._iq_ptr(iq_flat), C.c_void_p(offsets.data_ptr()),
                                                 C.c_void_p(counts.data_ptr()), int(max_samples), C.c_void_p(soft.data_ptr()),
                                                 soft.shape[1], min(cap, soft.shape[1]), self._stream()), "mdemod_fe_process_device")
        return soft

    def process(self, iq, soft=None):
        """Front end + demodulator on one block per stream (as ``Demodulator.process``): returns soft int8 [n_streams, cap, 2];
        per-stream symbol counts in :meth:`status`."""
        n, off, cnt = self._uniform_rows(iq)
        base = iq.as_strided(((self.n_streams - 1) * (iq.stride(0) // 2) + n, 2), (2, 1))
        return self.process_ragged(base, off, cnt, n, soft)

    def process_host(self, blocks):
        """Host buffers in and out (synchronous): one numpy [n_s, 2] block per stream, one int8 [m_s, 2] array per stream."""
        assert len(blocks) == self.n_streams
        dt = {8: np.uint8, 16: np.int16, 32: np.float32}[self.cfg.bps]
        blocks = [np.ascontiguousarray(b, dtype=dt).reshape(-1, 2) for b in blocks]
        ns = self.n_streams
        iq_ptrs = (C.c_void_p * ns)(*[b.ctypes.data for b in blocks])
        counts = (C.c_uint32 * ns)(*[b.shape[0] for b in blocks])
        caps = [self.max_symbols(b.shape[0]) for b in blocks]
        outs = [np.empty((c, 2), dtype=np.int8) for c in caps]
        soft_ptrs = (C.c_void_p * ns)(*[o.ctypes.data for o in outs])
        soft_caps = (C.c_uint32 * ns)(*caps)
        produced = (C.c_uint32 * ns)()
        check(self._lib.mdemod_fe_process_host(self._h, iq_ptrs, counts, soft_ptrs, soft_caps, produced), "mdemod_fe_process_host")
        return [o[:produced[i]] for i, o in enumerate(outs)]

    # -- the inner demodulator -------------------------------------------------
    def status(self, first: int = 0, count: int | None = None) -> list[MdemodStatus]:
        count = self.n_streams - first if count is None else count
        out = (MdemodStatus * count)()
        check(_capi.lib().mdemod_get_status(self._ctx, first, count, out, self._stream()), "mdemod_get_status")
        return list(out)

    def lock_events(self, stream: int) -> list[tuple[int, int]]:
        out = (MdemodLockEvent * _capi.MDEMOD_MAX_LOCK_EVENTS)()
        n = C.c_uint32()
        check(_capi.lib().mdemod_get_lock_events(self._ctx, stream, out, _capi.MDEMOD_MAX_LOCK_EVENTS, C.byref(n), self._stream()),
              "mdemod_get_lock_events")
        return [(out[i].symbol, out[i].locked) for i in range(n.value)]

    @property
    def kernel_name(self) -> str:
        return _capi.lib().mdemod_kernel_name(self._ctx).decode()


def demodulate_recording_frontend(cfg: DemodConfig, fe: FrontEndConfig, iq, device: int = 0, **opts):
    """ONE recording (device tensor [n, 2] in the input's format): the baseband on the device, then the existing
    ``mdemod_demodulate_recording`` on it (``recording.demodulate_recording_native`` with samplerate / D, f32).
    Returns (soft int8 [m, 2] device tensor, report)."""
    from .recording import demodulate_recording_native
    with FrontEnd(cfg, fe, 1, device=device) as f:
        bb, n_out = f.baseband(iq.reshape(1, -1, 2))
        base = bb[0, : int(n_out[0])].contiguous()
    return demodulate_recording_native(output_config(cfg, fe), base, device=device, **opts)


def demodulate_recording_frontend_host(cfg: DemodConfig, fe: FrontEndConfig, iq_host: np.ndarray, soft_capacity: int = 0, **opts):
    """``mdemod_fe_demodulate_recording_host`` (the CLI's --tiled path): host [n, 2] array in, (soft int8 [m, 2], report) out."""
    dt = {8: np.uint8, 16: np.int16, 32: np.float32}[cfg.bps]
    iq_host = np.ascontiguousarray(iq_host, dtype=dt).reshape(-1, 2)
    n = iq_host.shape[0]
    o = _capi.MdemodRecordingOpts()
    _capi.lib().mdemod_recording_default_opts(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    cap = int(soft_capacity) or int(n / fe.decimation * cfg.symrate / (cfg.samplerate / fe.decimation) * 1.05) + 65536
    soft = np.empty((cap, 2), dtype=np.int8)
    rep = MdemodRecordingReport()
    p = cfg.to_c(1)
    fp, _keep = fe.to_c()
    check(lib().mdemod_fe_demodulate_recording_host(C.byref(p), C.byref(fp), C.byref(o), iq_host.ctypes.data, n, soft.ctypes.data, cap,
                                                    C.byref(rep)), "mdemod_fe_demodulate_recording_host")
    return soft[: rep.n_symbols], rep
