"""The image layer: include/meteor_demod_amd_image.h over ctypes.

``find`` demultiplexes the packet zone of VCDUs (892 bytes each) into CCSDS space packets, ``decode`` turns the MSU-MR image
packets among them into strips of 8 x 112 pixels, both on the GPU with device tensors in and out; ``place`` says where each strip
belongs and ``paint`` puts them there.  ``vcdu_to_image`` and ``soft_to_image`` chain the steps (the second from soft symbols,
through ``rs.soft_to_vcdu``) without leaving the device before the strips; ``decode_file`` reads a ``.vcdu`` file.  ``model_*`` is
the host model of csrc/image_host.cpp, the kernels' specification.  This module keeps its own binding table, as ``rs.py`` does.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from ._capi import check, take_bytes

VCDU_BYTES, ZONE, STRIP_BYTES, WIDTH, CELLS, OVERLAP, MAX_PER_FRAME = 892, 882, 896, 1568, 14, 76, 126
NOT_IMAGE, BAD_HEADER, TRUNCATED, OUTSIDE = 1, 2, 4, 8

DESC_DTYPE = np.dtype([("start", "<u4"), ("length", "<u4"), ("apid", "<u2"), ("seq", "<u2"), ("flags", "<u4")])
SINFO_DTYPE = np.dtype([("mcus", "u1"), ("q", "u1"), ("mcun", "u1"), ("flags", "u1"), ("day", "<u2"), ("us", "<u2"), ("ms", "<u4"), ("bits_used", "<u4")])
PLACE_DTYPE = np.dtype([("channel", "<i4"), ("row", "<u4"), ("cell", "<u4"), ("reserved", "<u4")])


class MdemodImageOpts(C.Structure):
    _fields_ = [("vcid", C.c_uint32), ("period", C.c_uint32), ("apids", C.c_uint32 * 3), ("reserved", C.c_uint32), ("piece_frames", C.c_uint64)]


class MdemodPlaceSummary(C.Structure):
    _fields_ = [("packets", C.c_uint64), ("per_apid", C.c_uint64 * 6), ("placed", C.c_uint64), ("truncated", C.c_uint64), ("dropped", C.c_uint64),
                ("seq_gaps", C.c_uint64), ("cells_filled", C.c_uint64), ("first", C.c_int64), ("rows", C.c_uint32), ("anchored", C.c_uint32)]


class MdemodImageResult(C.Structure):
    _fields_ = [("n_packets", C.c_uint64), ("desc", C.c_void_p), ("sinfo", C.c_void_p), ("strips", C.c_void_p), ("place", C.c_void_p),
                ("summary", MdemodPlaceSummary), ("image", C.c_void_p * 3), ("filled", C.c_void_p * 3)]


_P = C.POINTER
# name -> (restype, argtypes): every entry of include/meteor_demod_amd_image.h
SIGNATURES = {
    "mdemod_image_default_opts": (None, [_P(MdemodImageOpts)]),
    "mdemod_packets_find_device": (C.c_int, [_P(MdemodImageOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_image_decode_device": (C.c_int, [_P(MdemodImageOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mdemod_image_place": (C.c_int, [_P(MdemodImageOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, _P(MdemodPlaceSummary)]),
    "mdemod_image_decode_host": (C.c_int, [_P(MdemodImageOpts), C.c_void_p, C.c_void_p, C.c_uint64, _P(MdemodImageResult), C.c_int]),
    "mdemod_image_free": (None, [_P(MdemodImageResult)]),
}
# the host model (csrc/image_host.h): exported for the tests
MODEL_SIGNATURES = {
    "mdemod_image_model_find": (C.c_int, [_P(MdemodImageOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "mdemod_image_model_decode": (C.c_int, [_P(MdemodImageOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mdemod_image_model_quant": (None, [C.c_uint32, C.c_void_p]),
    "mdemod_image_model_idct": (None, [C.c_void_p, C.c_void_p]),
    "mdemod_image_model_tables": (None, [C.c_void_p] * 6),
    "mdemod_image_model_encode_packet": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                     C.c_uint64]),
    "mdemod_image_model_host": (C.c_int, [_P(MdemodImageOpts), C.c_void_p, C.c_void_p, C.c_uint64, _P(MdemodImageResult)]),
}

@functools.cache
def lib() -> C.CDLL:
    """The product library with this layer's entries typed (the same handle as ``_capi.lib()``)."""
    return _capi.bind(SIGNATURES, MODEL_SIGNATURES)


def make_opts(**opts) -> MdemodImageOpts:
    """``mdemod_image_default_opts`` with the given fields replaced (an unknown name is a TypeError); ``apids`` takes three numbers."""
    o = MdemodImageOpts()
    lib().mdemod_image_default_opts(C.byref(o))
    names = {f[0] for f in MdemodImageOpts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"image: no option {k!r} (there are: {', '.join(sorted(names))})")
        if k == "apids":
            v = [int(x) for x in v]
            if len(v) != 3:
                raise ValueError("image: apids takes three numbers")
            o.apids[:] = v
        else:
            setattr(o, k, int(v))
    return o


@dataclass
class Result:
    """Packets, strips and pictures of a batch of VCDUs: ``desc`` / ``sinfo`` / ``place`` are structured arrays (DESC_DTYPE,
    SINFO_DTYPE, PLACE_DTYPE), ``strips`` is uint8 [n, 8, 112], ``images`` / ``filled`` map an active APID to uint8 [8 rows, 1568]
    and bool [rows, 14]."""
    desc: np.ndarray
    sinfo: np.ndarray
    strips: np.ndarray
    place: np.ndarray
    summary: dict
    images: dict = field(default_factory=dict)
    filled: dict = field(default_factory=dict)


@dataclass
class Report:
    """What ``decode_file`` says about a ``.vcdu`` file."""
    frames: int
    packets: int
    packets_per_apid: dict
    strips_placed: int
    strips_truncated: int
    strips_dropped: int
    lines_per_channel: dict
    sequence_gaps: int
    cells_filled: int


def _host_vcdu(vcdu) -> np.ndarray:
    a = np.ascontiguousarray(vcdu, dtype=np.uint8)
    if a.size % VCDU_BYTES:
        raise ValueError("VCDUs are 892 bytes each")
    return a.reshape(-1, VCDU_BYTES)


def _host_info(info, n):
    if info is None:
        return None
    a = np.ascontiguousarray(info, dtype=np.uint8).reshape(-1, 8)
    if a.shape[0] != n:
        raise ValueError(f"{a.shape[0]} reports for {n} frames")
    return a


def _check_dev(vcdu):
    import torch
    if not getattr(vcdu, "is_cuda", False):
        raise ValueError("vcdu must be a device tensor")
    if vcdu.dtype != torch.uint8 or vcdu.dim() != 2 or vcdu.shape[1] != VCDU_BYTES or not vcdu.is_contiguous():
        raise ValueError(f"vcdu must be a contiguous uint8 [n, 892] tensor, got {vcdu.dtype} {tuple(vcdu.shape)}")
    return vcdu.device.index or 0, int(vcdu.shape[0])


def find(vcdu, info=None, **opts):
    """VCDUs (uint8 [n, 892] device tensor) and their reports (uint8 [n, 8] device tensor as ``rs.decode`` leaves it, or None:
    all frames good) to the descriptors of the accepted packets: a uint8 [total, 16] device tensor (``descriptors`` reads it).
    Queued on the current stream; the total is read back once, to size the result."""
    import torch
    o = make_opts(**opts)
    dev, n = _check_dev(vcdu)
    if info is not None and (not info.is_cuda or info.dtype != torch.uint8 or info.numel() != 8 * n or not info.is_contiguous()):
        raise ValueError("info must be a contiguous uint8 [n, 8] device tensor")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cap = MAX_PER_FRAME * n
    desc = torch.zeros((cap, 16), dtype=torch.uint8, device=vcdu.device)
    total = torch.zeros(1, dtype=torch.int64, device=vcdu.device)
    check(lib().mdemod_packets_find_device(C.byref(o), C.c_void_p(vcdu.data_ptr()), C.c_void_p(info.data_ptr()) if info is not None else None, n,
                                           C.c_void_p(desc.data_ptr()), cap, C.c_void_p(total.data_ptr()), dev, st), "mdemod_packets_find_device")
    return desc[: int(total.item())].clone()


def decode(vcdu, desc, **opts):
    """Descriptors (uint8 [m, 16] device tensor) over VCDUs to (strips uint8 [m, 8, 112], reports uint8 [m, 16]), device tensors."""
    import torch
    o = make_opts(**opts)
    dev, n = _check_dev(vcdu)
    if not desc.is_cuda or desc.dtype != torch.uint8 or desc.dim() != 2 or desc.shape[1] != 16 or not desc.is_contiguous():
        raise ValueError("desc must be a contiguous uint8 [m, 16] device tensor")
    m = int(desc.shape[0])
    strips = torch.zeros((m, 8, 112), dtype=torch.uint8, device=vcdu.device)
    sinfo = torch.zeros((m, 16), dtype=torch.uint8, device=vcdu.device)
    check(lib().mdemod_image_decode_device(C.byref(o), C.c_void_p(vcdu.data_ptr()), n, C.c_void_p(desc.data_ptr()), m, C.c_void_p(strips.data_ptr()),
                                           C.c_void_p(sinfo.data_ptr()), dev, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mdemod_image_decode_device")
    return strips, sinfo


def _structured(raw, dtype) -> np.ndarray:
    a = raw.cpu().numpy() if hasattr(raw, "cpu") else np.asarray(raw)
    if a.dtype == dtype:
        return np.ascontiguousarray(a).reshape(-1)
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 16).view(dtype).reshape(-1)


def descriptors(raw) -> np.ndarray:
    """uint8 [m, 16] (tensor or array) as a structured array of DESC_DTYPE."""
    return _structured(raw, DESC_DTYPE)


def strip_infos(raw) -> np.ndarray:
    """uint8 [m, 16] (tensor or array) as a structured array of SINFO_DTYPE."""
    return _structured(raw, SINFO_DTYPE)


def _summary(s: MdemodPlaceSummary) -> dict:
    return dict(packets=int(s.packets), per_apid={64 + k: int(s.per_apid[k]) for k in range(6)}, placed=int(s.placed), truncated=int(s.truncated),
                dropped=int(s.dropped), seq_gaps=int(s.seq_gaps), cells_filled=int(s.cells_filled), first=int(s.first), rows=int(s.rows),
                anchored=bool(s.anchored))


def place(desc, sinfo, **opts):
    """``mdemod_image_place``: (structured array of PLACE_DTYPE, summary dict) for descriptors and strip reports (structured or raw)."""
    o = make_opts(**opts)
    d, s = descriptors(desc), strip_infos(sinfo)
    if len(d) != len(s):
        raise ValueError(f"{len(d)} descriptors and {len(s)} reports")
    out = np.zeros(len(d), dtype=PLACE_DTYPE)
    summ = MdemodPlaceSummary()
    check(lib().mdemod_image_place(C.byref(o), d.ctypes.data, s.ctypes.data, len(d), out.ctypes.data, C.byref(summ)), "mdemod_image_place")
    return out, _summary(summ)


def paint(strips, placement, rows: int, apids=(64, 65, 66)):
    """The pictures and the masks of the placed strips: ({apid: uint8 [8 rows, 1568]}, {apid: bool [rows, 14]})."""
    st = np.asarray(strips, dtype=np.uint8).reshape(-1, 8, 112)
    images = {a: np.zeros((8 * rows, WIDTH), dtype=np.uint8) for a in apids}
    filled = {a: np.zeros((rows, CELLS), dtype=bool) for a in apids}
    for i, p in enumerate(placement):
        if p["channel"] < 0:
            continue
        a, r, c = apids[int(p["channel"])], int(p["row"]), int(p["cell"])
        images[a][8 * r: 8 * r + 8, 112 * c: 112 * c + 112] = st[i]
        filled[a][r, c] = True
    return images, filled


def _finish(desc, sinfo, strips, o: MdemodImageOpts) -> Result:
    apids = tuple(int(a) for a in o.apids)
    pl, summ = place(desc, sinfo, vcid=o.vcid, period=o.period, apids=apids)
    images, filled = paint(strips, pl, summ["rows"], apids)
    summ["cells_filled"] = int(sum(f.sum() for f in filled.values()))
    return Result(descriptors(desc), strip_infos(sinfo), np.asarray(strips, dtype=np.uint8).reshape(-1, 8, 112), pl, summ, images, filled)


def vcdu_to_image(vcdu, info=None, **opts) -> Result:
    """VCDUs to pictures.  Device tensors go through ``find`` and ``decode`` on the device and only the descriptors, the strips and
    their reports come to the host for the placement; numpy arrays go through ``mdemod_image_decode_host``, copied in pieces of
    ``piece_frames`` (``device`` says where)."""
    device = int(opts.pop("device", 0))
    o = make_opts(**opts)
    if isinstance(vcdu, np.ndarray):
        a = _host_vcdu(vcdu)
        i = _host_info(info, a.shape[0])
        res = MdemodImageResult()
        check(lib().mdemod_image_decode_host(C.byref(o), a.ctypes.data, i.ctypes.data if i is not None else None, a.shape[0], C.byref(res), device),
              "mdemod_image_decode_host")
        return _take(res, o)
    dev_opts = {k: v for k, v in opts.items() if k != "piece_frames"}
    desc = find(vcdu, info, **dev_opts)
    strips, sinfo = decode(vcdu, desc, **dev_opts)
    return _finish(desc.cpu().numpy(), sinfo.cpu().numpy(), strips.cpu().numpy(), o)


def _take(res: MdemodImageResult, o: MdemodImageOpts) -> Result:
    """A C result into arrays of our own; the C side's memory goes back."""
    try:
        m, rows = int(res.n_packets), int(res.summary.rows)
        out = Result(take_bytes(res.desc, m, DESC_DTYPE), take_bytes(res.sinfo, m, SINFO_DTYPE), take_bytes(res.strips, m * STRIP_BYTES).reshape(-1, 8, 112),
                     take_bytes(res.place, m, PLACE_DTYPE), _summary(res.summary))
        for k in range(3):
            a = int(o.apids[k])
            out.images[a] = take_bytes(res.image[k], rows * 8 * WIDTH).reshape(8 * rows, WIDTH)
            out.filled[a] = take_bytes(res.filled[k], rows * CELLS).reshape(rows, CELLS).astype(bool)
        return out
    finally:
        lib().mdemod_image_free(C.byref(res))


def soft_to_image(soft, **opts):
    """Soft symbols (int8 [m, 2] device tensor) to (``Result``, the frame list): ``rs.soft_to_vcdu`` -> ``find`` -> ``decode`` ->
    placement.  Symbols, CADUs, VCDUs and strips stay on the device; the descriptors' total and the final strips and reports come
    to the host.  Options: ``vcid``, ``period``, ``apids`` go to this layer, the rest to ``rs.soft_to_vcdu``."""
    from . import rs
    mine = {k: opts.pop(k) for k in ("vcid", "period", "apids") if k in opts}
    vcdu, info, found = rs.soft_to_vcdu(soft, **opts)
    return vcdu_to_image(vcdu, info, **mine), found


def decode_file(path, **opts):
    """A ``.vcdu`` file (every frame taken as good: the file carries no reports) to (``Result``, ``Report``)."""
    raw = np.fromfile(str(path), dtype=np.uint8)
    vcdu = raw[: raw.size // VCDU_BYTES * VCDU_BYTES].reshape(-1, VCDU_BYTES)
    res = vcdu_to_image(vcdu, None, **opts)
    return res, report(res, len(vcdu))


def report(res: Result, frames: int) -> Report:
    per = {}
    for a in res.desc["apid"]:
        per[int(a)] = per.get(int(a), 0) + 1
    s = res.summary
    return Report(frames, len(res.desc), per, s["placed"], s["truncated"], s["dropped"], {a: int(im.shape[0]) for a, im in res.images.items()},
                  s["seq_gaps"], s["cells_filled"])


# ------------------------------------------------------------------------------------------------------------- the host model
def model_find(vcdu, info=None, **opts) -> np.ndarray:
    a = _host_vcdu(vcdu)
    i = _host_info(info, a.shape[0])
    o = make_opts(**opts)
    cap = MAX_PER_FRAME * a.shape[0]
    desc = np.zeros(max(cap, 1), dtype=DESC_DTYPE)
    total = C.c_uint64(0)
    check(lib().mdemod_image_model_find(C.byref(o), a.ctypes.data, i.ctypes.data if i is not None else None, a.shape[0], desc.ctypes.data, cap, C.byref(total)),
          "mdemod_image_model_find")
    return desc[: total.value].copy()


def model_decode(vcdu, desc, **opts):
    """(uint8 [m, 8, 112], structured reports [m]) of the host model."""
    a = _host_vcdu(vcdu)
    d = descriptors(desc)
    o = make_opts(**opts)
    strips, sinfo = np.zeros((len(d), 8, 112), dtype=np.uint8), np.zeros(len(d), dtype=SINFO_DTYPE)
    check(lib().mdemod_image_model_decode(C.byref(o), a.ctypes.data, a.shape[0], d.ctypes.data, len(d), strips.ctypes.data, sinfo.ctypes.data),
          "mdemod_image_model_decode")
    return strips, sinfo


def model_quant(q: int) -> np.ndarray:
    out = np.zeros(64, dtype=np.uint16)
    lib().mdemod_image_model_quant(int(q), out.ctypes.data)
    return out


def model_idct(coef) -> np.ndarray:
    a = np.ascontiguousarray(coef, dtype=np.int32).reshape(64)
    out = np.zeros(64, dtype=np.uint8)
    lib().mdemod_image_model_idct(a.ctypes.data, out.ctypes.data)
    return out.reshape(8, 8)


def model_tables() -> dict:
    bits, dc, ac, zz, sq, m = (np.zeros(32, np.uint8), np.zeros(12, np.uint8), np.zeros(162, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.uint8),
                               np.zeros(64, np.int32))
    lib().mdemod_image_model_tables(bits.ctypes.data, dc.ctypes.data, ac.ctypes.data, zz.ctypes.data, sq.ctypes.data, m.ctypes.data)
    return dict(dc_bits=bits[:16], ac_bits=bits[16:], dc_val=dc, ac_val=ac, zigzag=zz, std=sq, m=m.reshape(8, 8))


def model_encode_packet(strip, q: int, mcun: int, apid: int, seq: int, day: int = 0, ms: int = 0, us: int = 0) -> bytes:
    """The synthetic sender: one uint8 [8, 112] strip to the bytes of a whole packet."""
    a = np.ascontiguousarray(strip, dtype=np.uint8)
    if a.shape != (8, 112):
        raise ValueError("a strip is 8 x 112")
    out = np.zeros(65542, dtype=np.uint8)
    n = lib().mdemod_image_model_encode_packet(a.ctypes.data, q, mcun, apid, seq, day, ms, us, out.ctypes.data, out.size)
    if n < 0:
        check(int(n), "mdemod_image_model_encode_packet")
    return out[:n].tobytes()


def model_host(vcdu, info=None, **opts) -> Result:
    """``mdemod_image_decode_host`` with the model in the kernels' place (no device): the pieces and the placement."""
    a = _host_vcdu(vcdu)
    i = _host_info(info, a.shape[0])
    o = make_opts(**opts)
    res = MdemodImageResult()
    check(lib().mdemod_image_model_host(C.byref(o), a.ctypes.data, i.ctypes.data if i is not None else None, a.shape[0], C.byref(res)), "mdemod_image_model_host")
    return _take(res, o)
