"""What the modules of the two encoders (jpeg.py, png.py) share: the checks of a picture, the scratch memory and the result protocol of
a device entry, the call of a host entry, the file on disk.  The entries themselves and their binding tables stay in the modules."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._capi import check, take_bytes


def picture(picture, valid=None) -> tuple:
    """(contiguous uint8 picture, contiguous uint8 mask or None, width, height, planes) of numpy arrays."""
    px = np.ascontiguousarray(picture, dtype=np.uint8)
    if px.ndim == 2:
        planes = 1
    elif px.ndim == 3 and px.shape[2] in (1, 3):
        planes = int(px.shape[2])
    else:
        raise ValueError(f"a picture is uint8 [H, W] or [H, W, 3], got {tuple(px.shape)}")
    va = None
    if valid is not None:
        va = np.ascontiguousarray(valid, dtype=np.uint8)
        if va.shape != px.shape[:2]:
            raise ValueError(f"the mask of a picture {tuple(px.shape)} is uint8 [H, W], got {tuple(va.shape)}")
    return px, va, int(px.shape[1]), int(px.shape[0]), planes


def tensor(picture) -> tuple:
    """(width, height, planes) of a contiguous uint8 tensor [H, W], [H, W, 1] or [H, W, 3] on the GPU."""
    import torch
    if picture.dtype != torch.uint8 or not picture.is_contiguous() or not picture.is_cuda:
        raise ValueError("the picture must be a contiguous uint8 tensor on the GPU")
    if picture.dim() == 2:
        planes = 1
    elif picture.dim() == 3 and picture.shape[2] in (1, 3):
        planes = int(picture.shape[2])
    else:
        raise ValueError(f"a picture is uint8 [H, W] or [H, W, 3], got {tuple(picture.shape)}")
    return int(picture.shape[1]), int(picture.shape[0]), planes


class Scratch:
    """A device entry's side of the call on the device of the tensor ``like`` and its current stream: an output of ``room`` bytes, a
    workspace of ``need`` bytes and the two result words."""

    def __init__(self, like, room: int, need: int):
        import torch
        dev = like.device
        self.d = dev.index or 0
        self.stream = C.c_void_p(torch.cuda.current_stream(self.d).cuda_stream)
        self.out = torch.empty(max(room, 1), dtype=torch.uint8, device=dev)
        self.work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        self.result = torch.zeros(2, dtype=torch.int64, device=dev)
        # what every device entry ends in: out_dev, out_room, result_dev, work_dev, work_bytes, device, hip_stream
        self.tail = (C.c_void_p(self.out.data_ptr()), room, C.c_void_p(self.result.data_ptr()), C.c_void_p(self.work.data_ptr()), need, self.d, self.stream)

    def finish(self, result_entry, name: str) -> bytes:
        """The bytes that the entry left, through the layer's ``*_result`` entry (a ``MdemodError`` when they did not fit)."""
        n = C.c_uint64()
        check(result_entry(C.c_void_p(self.result.data_ptr()), C.byref(n), self.d, self.stream), name)
        return self.out[: n.value].cpu().numpy().tobytes()


def host_call(entry, name: str, free, head, device: int) -> bytes:
    """A ``*_encode_host`` entry: the arguments ``head``, then file, bytes and device; the file is copied and given back through ``free``."""
    file, n = C.c_void_p(), C.c_uint64()
    check(entry(*head, C.byref(file), C.byref(n), int(device)), name)
    try:
        return take_bytes(file.value, n.value).tobytes()
    finally:
        free(file)


def write(path, data: bytes) -> int:
    with open(os.fspath(path), "wb") as f:
        f.write(data)
    return len(data)
