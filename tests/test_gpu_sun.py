"""GPU tests of the sun layer (include/meteor_demod_amd_sun.h): the apply kernel against the host model, bytes and saturation
totals, at 1, 3 and 77 strip rows (one block, three blocks, and more blocks than a wave of them with a row count that is no
multiple of anything), slot masks 1, 5 and 7, out of place and in place, on the gain tables of a daytime pass, of a pass across the
terminator and of a synthetic table with missing nodes on every edge of a cell, over random pictures that hold 0 and 255; outputs
and the workspace inside canaries, inputs and unselected slots untouched; the device entry's refusals; the host and Python entries;
and a truth check on a scene that is the cosine of the sun's zenith angle itself.  Every GPU step runs once; every test prints the
figures it asserts on."""
from __future__ import annotations

import ctypes as C
import functools
import re

import numpy as np
import pytest

import map_util as M
import sun_ref as S
import sun_util as U

pytestmark = pytest.mark.gpu

PAD = 4096                              # canary bytes before and behind every buffer (a multiple of 4: the buffers stay on dwords)
CANARY, WORK_CANARY = 0xC3, 0x5EED5EED
MASKS = (1, 5, 7)


@functools.lru_cache(maxsize=None)
def _model(rows: int, kind: str, mask: int):
    """The host model's pictures and counts of a case: computed once, not to be changed."""
    from meteor_demod_amd import sun
    out, sat = sun.model_apply(U.pictures(rows), U.gain_table(kind, rows), mask)
    for k in range(3):
        if mask >> k & 1:
            out[k].setflags(write=False)
    return out, sat


def _padded(gpu_device, count: int, fill: int, dtype):
    """A device buffer of ``count`` elements between two canaries: (the whole tensor, the view between them)."""
    import torch
    pad = PAD // np.dtype(dtype).itemsize
    whole = torch.from_numpy(np.full(count + 2 * pad, fill, dtype=dtype)).to(f"cuda:{gpu_device}")
    return whole, whole[pad: pad + count]


def _canaries_intact(whole, count: int, fill: int) -> bool:
    a = whole.cpu().numpy()
    pad = (a.size - count) // 2
    return bool((a[:pad] == fill).all() and (a[pad + count:] == fill).all())


def _call(images, outs, mask, rows, gain, work, work_bytes, gpu_device):
    import torch
    from meteor_demod_amd import sun
    ptr = lambda t: t if isinstance(t, (int, type(None))) else t.data_ptr()      # a tensor, an address or None
    pi, po = (C.c_void_p * 3)(*[ptr(t) for t in images]), (C.c_void_p * 3)(*[ptr(t) for t in outs])
    return sun.lib().mdemod_sun_apply_device(C.byref(pi), C.byref(po), mask, rows, ptr(gain), ptr(work), work_bytes, gpu_device,
                                             C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream))


@pytest.mark.parametrize("kind", ["day", "terminator", "synthetic"])
@pytest.mark.parametrize("rows", [1, 3, 77])
def test_kernel_equals_model(rows, kind, gpu_device):
    import torch
    from meteor_demod_amd import sun
    pics, gain = U.pictures(rows), U.gain_table(kind, rows)
    area = 8 * rows * S.WIDTH
    d_gain = torch.from_numpy(gain.view(np.int32)).to(f"cuda:{gpu_device}")
    for mask in MASKS:
        want, wsat = _model(rows, kind, mask)
        for in_place in (False, True):
            ins = [_padded(gpu_device, area, CANARY, np.uint8) for _ in range(3)]
            for k in range(3):
                ins[k][1].copy_(torch.from_numpy(pics[k].reshape(-1)))
            outs = ins if in_place else [_padded(gpu_device, area, CANARY, np.uint8) for _ in range(3)]
            work_whole, work = _padded(gpu_device, 3 * rows, WORK_CANARY, np.int32)
            rc = _call([t[1] for t in ins], [t[1] for t in outs], mask, rows, d_gain, work, sun.workspace(rows), gpu_device)
            assert rc == 0, sun._capi.last_error()
            torch.cuda.synchronize(gpu_device)
            what = (rows, kind, mask, "in place" if in_place else "out of place")
            for k in range(3):
                got = outs[k][1].cpu().numpy().reshape(8 * rows, S.WIDTH)
                if mask >> k & 1:
                    assert np.array_equal(got, want[k]), (what, k, int((got != want[k]).sum()))
                elif in_place:
                    assert np.array_equal(got, pics[k]), (what, k)                  # a slot that is not selected is not touched
                else:
                    assert (got == CANARY).all(), (what, k)
                assert _canaries_intact(outs[k][0], area, CANARY), (what, k)
                if not in_place:
                    assert np.array_equal(ins[k][1].cpu().numpy().reshape(8 * rows, S.WIDTH), pics[k]) and _canaries_intact(ins[k][0], area, CANARY), (what, k)
            counts = work.cpu().numpy().view(np.uint32).reshape(rows, 3).astype(np.int64)
            sat = [int(v) for v in counts.sum(axis=0)]
            assert sat == wsat and counts.max() <= 8 * S.WIDTH, (what, sat, wsat)
            assert _canaries_intact(work_whole, 3 * rows, WORK_CANARY), what
        print(f"rows {rows} {kind} mask {mask}: saturated {wsat}, {sum(int((want[k] != pics[k]).sum()) for k in range(3) if mask >> k & 1)} bytes changed")
    assert np.array_equal(d_gain.cpu().numpy().view(np.uint32), gain)


def test_device_entry_refusals(gpu_device):
    """Every refusal has its code and text, and nothing is written."""
    import torch
    from meteor_demod_amd import _capi, sun
    rows = 2
    area = 8 * rows * S.WIDTH
    pics = U.pictures(rows)
    ins = [torch.from_numpy(p.reshape(-1).copy()).to(f"cuda:{gpu_device}") for p in pics]
    room = torch.from_numpy(np.full(3 * area + 64, CANARY, np.uint8)).to(f"cuda:{gpu_device}")
    outs = [room[k * area: (k + 1) * area] for k in range(3)]
    gain = torch.from_numpy(U.synthetic_gain(rows).view(np.int32)).to(f"cuda:{gpu_device}")
    work = torch.full((3 * rows + 4,), 0x11111111, dtype=torch.int32, device=f"cuda:{gpu_device}")
    need = sun.workspace(rows)
    assert need == 12 * rows
    cases = [
        (lambda: _call(ins, outs, 7, 0, gain, work, need, gpu_device), r"0 strip rows are outside 1 \.\. 8192"),
        (lambda: _call(ins, outs, 7, 8193, gain, work, 1 << 20, gpu_device), r"8193 strip rows"),
        (lambda: _call(ins, outs, 0, rows, gain, work, need, gpu_device), r"slot mask 0 is outside 1 \.\. 7"),
        (lambda: _call(ins, outs, 9, rows, gain, work, need, gpu_device), r"slot mask 9 is outside 1 \.\. 7"),
        (lambda: _call(ins, outs, 7, rows, None, work, need, gpu_device), r"gain table is needed"),
        (lambda: _call(ins, outs, 7, rows, gain, None, need, gpu_device), r"workspace is needed"),
        (lambda: _call(ins, outs, 7, rows, gain, work, need - 1, gpu_device), rf"workspace needs {need} bytes, not {need - 1}"),
        (lambda: _call([ins[0], ins[1], None], outs, 7, rows, gain, work, need, gpu_device), r"slot 2 are needed"),
        (lambda: _call(ins, [None, outs[1], outs[2]], 1, rows, gain, work, need, gpu_device), r"slot 0 are needed"),
        (lambda: _call(ins, [outs[0].data_ptr() + 2, outs[1], outs[2]], 1, rows, gain, work, need, gpu_device), r"multiples of 4 bytes"),
        (lambda: _call([ins[0].data_ptr() + 1, ins[1], ins[2]], outs, 1, rows, gain, work, need, gpu_device), r"multiples of 4 bytes"),
        (lambda: _call(ins, outs, 1, rows, gain.data_ptr() + 2, work, need, gpu_device), r"multiples of 4 bytes"),
        (lambda: _call(ins, [outs[0], outs[0].data_ptr() + 4, outs[2]], 3, rows, gain, work, need, gpu_device), r"intersect"),
        (lambda: _call(ins, [ins[1], outs[1], outs[2]], 3, rows, gain, work, need, gpu_device), r"intersect"),
        (lambda: _call([outs[0].data_ptr() + 4, ins[1], ins[2]], outs, 1, rows, gain, work, need, gpu_device), r"intersect"),
        (lambda: _call(ins, [gain, outs[1], outs[2]], 1, rows, gain, work, need, gpu_device), r"intersect"),
        (lambda: _call(ins, outs, 1, rows, gain, outs[0], need, gpu_device), r"intersect"),
    ]
    for call, pattern in cases:
        rc = call()
        text = _capi.last_error()
        print(f"  {rc}: {text}")
        assert rc == -1 and re.search(pattern, text), (rc, text, pattern)
    torch.cuda.synchronize(gpu_device)
    assert (room.cpu().numpy() == CANARY).all() and (work.cpu().numpy() == 0x11111111).all()
    assert all(np.array_equal(ins[k].cpu().numpy(), pics[k].reshape(-1)) for k in range(3))
    # and the same call with everything in order goes through
    assert _call(ins, outs, 7, rows, gain, work, need, gpu_device) == 0
    torch.cuda.synchronize(gpu_device)
    assert not (room.cpu().numpy()[: 3 * area] == CANARY).all() and (room.cpu().numpy()[3 * area:] == CANARY).all()


def test_python_and_host_entries(gpu_device):
    """``apply`` on numpy arrays and on tensors with ``out=``; ``correct_images`` through mdemod_sun_correct_host against the model
    in the kernel's place, with a thermal channel in slot 1."""
    import torch
    from meteor_demod_amd import sun
    rows = 3
    pics, gain = U.pictures(rows), U.gain_table("terminator", rows)
    want, wsat = _model(rows, "terminator", 5)
    out, sat = sun.apply(pics, gain, slots=(0, 2), device=gpu_device)
    assert sat == wsat and out[1] is pics[1] and all(np.array_equal(out[k], want[k]) for k in (0, 2))
    tens = [torch.from_numpy(p).to(f"cuda:{gpu_device}") for p in pics]
    res, sat = sun.apply(tens, gain, slots=5, out=[tens[0], None, None])               # slot 0 in place, slot 2 into a new tensor
    assert sat == wsat and res[0] is tens[0] and res[1] is None and np.array_equal(res[0].cpu().numpy(), want[0]) and np.array_equal(res[2].cpu().numpy(), want[2])
    assert np.array_equal(tens[2].cpu().numpy(), pics[2])
    with pytest.raises(ValueError, match="gain table"):
        sun.apply(tens, gain[:-1], slots=1)
    rows = 6
    pics = U.pictures(rows)
    place, info = U.packets("terminator", rows)
    got, summ = sun.correct_images(pics, (64, 68, 66), place, info, M.tle_text(), device=gpu_device, **U.map_opts("terminator"))
    ref, rsumm = sun.correct_images(pics, (64, 68, 66), place, info, M.tle_text(), model=True, **U.map_opts("terminator"))
    print(summ)
    assert summ == rsumm and summ["slot_mask"] == 5 and summ["saturated"][0] > 0 and summ["saturated"][1] == 0
    assert all(np.array_equal(got[k], ref[k]) for k in range(3)) and np.array_equal(got[1], pics[1]) and not np.array_equal(got[0], pics[0])


def test_truth_a_scene_that_is_the_cosine_itself(gpu_device):
    """40 rows of the terminator pass, every pixel v = round(240 cos z) with cos z exact per pixel from sun_ref (not interpolated),
    the same in the three channels.  After ``correct`` (limit 85, reference 45) every pixel with z <= 84 lies within
    0.5 gain + 1 + m of 240 cos 45 = 169.7: half a level of the scene's rounding times the gain, one level for the rounding of the
    output and of the nodes, and m for the interpolation between nodes - twice the largest relative difference between the exact and
    the node-interpolated gain over these pixels, measured here with sun_ref on the CPU (profiles/sun.md records it), times 169.7.
    Without the correction the same picture spans more than 100 grey levels."""
    from meteor_demod_amd import image, sun
    rows, limit, ref_deg = 40, 85.0, 45.0
    ref = U.ref_pass("terminator")
    y, x = np.meshgrid(np.arange(8.0 * rows), np.arange(float(S.WIDTH)), indexing="ij")
    c = S.pass_cos_zenith(ref, y, x)
    assert np.isfinite(c).all()
    scene = np.clip(np.rint(240.0 * c), 0, 255).astype(np.uint8)
    z = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
    checked = z <= limit - 1.0
    exact = S.gain_of(c, limit, ref_deg) / 65536.0
    g, missing = S.pixel_gain(U.ref_nodes("terminator", rows, limit, ref_deg)[0], rows)
    assert not missing.any()
    rel = float((np.abs(g / 65536.0 - exact) / exact)[checked].max())
    target = 240.0 * np.cos(np.radians(ref_deg))
    m = 2.0 * rel * target
    place, info = U.packets("terminator", rows)
    res = image.Result(np.zeros(0), info, np.zeros((0, 8, 112), np.uint8), place, {}, {a: scene.copy() for a in (64, 65, 66)},
                       {a: np.ones((rows, 14), np.uint8) for a in (64, 65, 66)})
    out = sun.correct(res, M.tle_text(), device=gpu_device, limit_deg=limit, ref_deg=ref_deg, **U.map_opts("terminator"))
    span = int(scene.max()) - int(scene.min())
    print(f"zenith {z.min():.2f} .. {z.max():.2f}; {int(checked.sum())} of {checked.size} pixels at z <= {limit - 1}; the scene spans {span} grey levels "
          f"({int(scene[checked].max()) - int(scene[checked].min())} over the checked pixels); largest relative difference exact / interpolated gain {rel:.3e}, m = {m:.4f}")
    print(f"summary: {out.sun}")
    assert span > 100 and checked.sum() > 200000
    assert out.sun["slot_mask"] == 7 and list(out.images) == [64, 65, 66] and res.images[64] is not out.images[64] and np.array_equal(res.images[64], scene)
    for a in (64, 65, 66):
        err = np.abs(out.images[a].astype(np.float64) - target)
        slack = (0.5 * exact + 1.0 + m) - err
        after = out.images[a][checked]
        print(f"apid {a}: corrected {int(after.min())} .. {int(after.max())} around {target:.2f}; largest error {err[checked].max():.3f}, least slack {slack[checked].min():.3f}")
        assert (slack[checked] >= 0.0).all()
        assert int(after.max()) - int(after.min()) < span // 4
    assert np.array_equal(out.images[64], out.images[65]) and np.array_equal(out.images[64], out.images[66])
