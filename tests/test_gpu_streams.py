"""GPU tests of the stream contract of every device entry (tests/stream_cases.py: one row per exported function with a ``hip_stream``
parameter; the headers say "asynchronous on hip_stream" or "synchronous" of each).

Every other GPU test runs its entry on the null stream, where a launch that dropped its stream argument, a temporary freed before
its kernel ran, a table uploaded on another stream or a hidden device-wide wait still give the right bytes.  Here each entry runs on a
non-blocking side stream behind a delay kernel: the input buffers hold the poison (a second valid input), the output buffers a canary;
on the side stream are queued the delay, device-to-device copies of the real input into the input buffers, then the entry.  Whatever
part of the entry runs on another stream runs while the delay spins and reads the poison or is overwritten.  An asynchronous entry
must have returned while the delay was still running; a synchronous one hands back host memory that is right without a wait of the
test's.  The expectation is the host model's, never a GPU run's.

The instrument checks itself once per module: the same arrangement with mdemod_rs_decode_device given the NULL stream must produce the
model's result for the POISON - on this machine, work off the side stream does overtake the delay.  Side streams whose hardware queue
the null stream shares fail that and are passed over (up to eight); with none left the module fails instead of passing blind.

Every GPU step runs once per row.  The delay is at least 20 x the host time of the row's warm call (scheduling jitter must not make
an asynchronous call look synchronous), at least 50 ms and at most 500 ms; each row prints its t_call, the measured delay and the side stream."""
from __future__ import annotations

import contextlib
import ctypes as C
import time

import numpy as np
import pytest

import stream_cases as SC

pytestmark = pytest.mark.gpu

FACTOR, FLOOR_MS, CEILING_MS = 20.0, 50.0, 500.0           # (a delay is a few hundred milliseconds at the most)
MAX_STREAMS = 8
_FAULT = []                               # what a GPU fault said: after one, no later test of the module touches the GPU


def _no_fault_so_far():
    if _FAULT:
        pytest.fail(f"not run: an earlier test of this module met a GPU fault ({_FAULT[0]})")


def _note_fault(e: BaseException) -> None:
    text = str(e).lower()
    if "illegal memory access" in text or "hip error" in text or "hiperror" in text or "mdemod_err_hip" in text:
        _FAULT.append(str(e)[:200])


@contextlib.contextmanager
def _latched():
    """Around everything of this module that uses the GPU - the calibration and the control, every row, the chains: nothing starts
    after a fault, and a fault met inside is kept for the tests that follow."""
    _no_fault_so_far()
    try:
        yield
    except BaseException as e:
        _note_fault(e)
        raise


def _up(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)            # (a copy: the cases are read-only)


def _upload(row, host: dict, dev: str) -> dict:
    return {k: (np.array(v) if k in row.host_inputs else _up(v, dev)) for k, v in host.items()}


def _device_names(row, host: dict) -> list:
    return [k for k in host if k not in row.host_inputs]


def _fetch(outputs: list) -> list:
    """Device outputs to the host on the current stream; read-backs (callables) made; host results as they are."""
    got = []
    for o in outputs:
        if callable(o):
            o = o()
        got.append(o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o))
    return got


class Delay:
    """A spin kernel of a wanted length on the current stream, between two events."""

    def __init__(self, cycles_per_ms: float):
        self.cycles_per_ms = cycles_per_ms

    def queue(self, ms: float):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(int(1.15 * ms * self.cycles_per_ms))
        e1.record()
        return e0, e1


def _calibrate(side) -> float:
    """Spin cycles per millisecond, from two events on the side stream."""
    import torch
    with torch.cuda.stream(side):
        torch.cuda._sleep(1000)                                                   # (its code object)
        side.synchronize()
        cycles = 20_000_000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        side.synchronize()
    return cycles / e0.elapsed_time(e1)


def _control(side, delay: Delay, gpu_device: int):
    """mdemod_rs_decode_device on the NULL stream while the side stream holds delay + copies of the real input: (what it wrote, whether
    the delay was still running when the null stream had finished)."""
    import torch
    from meteor_demod_amd import rs
    dev = f"cuda:{gpu_device}"
    real, poison = SC.case("mdemod_rs_decode_device", "real"), SC.case("mdemod_rs_decode_device", "poison")
    n = real["cadu"].shape[0]
    buf, src = _up(poison["cadu"], dev), _up(real["cadu"], dev)
    vcdu = torch.full((n, 892), SC.CANARY, dtype=torch.uint8, device=dev)
    info = torch.full((n, 8), SC.CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.stream(side):
        e0, e1 = delay.queue(2 * FLOOR_MS)
        buf.copy_(src)
    rc = rs.lib().mdemod_rs_decode_device(None, C.c_void_p(buf.data_ptr()), n, C.c_void_p(vcdu.data_ptr()), C.c_void_p(info.data_ptr()), gpu_device, None)
    assert rc == 0
    torch.cuda.default_stream(gpu_device).synchronize()
    overtook = not e1.query()
    got = [vcdu.cpu().numpy(), info.cpu().numpy()]
    side.synchronize()
    return got, overtook, e0.elapsed_time(e1)


@pytest.fixture(scope="module")
def instrument(gpu_device):
    """(side stream, Delay) for the module: the first stream of torch's pool, of up to eight, on which the control holds."""
    with _latched():
        return _instrument(gpu_device)


def _instrument(gpu_device):
    import torch
    assert hasattr(torch.cuda, "_sleep"), "this torch build has no torch.cuda._sleep"
    torch.cuda.set_device(gpu_device)
    want_poison = list(SC.want("mdemod_rs_decode_device", "poison"))
    want_real = list(SC.want("mdemod_rs_decode_device", "real"))
    seen = []
    for k in range(MAX_STREAMS):
        side = torch.cuda.Stream(gpu_device)
        delay = Delay(_calibrate(side))
        got, overtook, ms = _control(side, delay, gpu_device)
        is_poison = all(np.array_equal(g, w) for g, w in zip(got, want_poison))
        is_real = all(np.array_equal(g, w) for g, w in zip(got, want_real))
        seen.append((k, hex(side.cuda_stream), overtook, "poison" if is_poison else "real" if is_real else "neither"))
        print(f"control, side stream {k} ({hex(side.cuda_stream)}): {delay.cycles_per_ms:.0f} spin cycles per ms, delay {ms:.1f} ms; the null-stream call "
              f"{'overtook the delay' if overtook else 'waited for the delay'} and wrote the model's result for the {seen[-1][3]} input")
        assert is_poison or is_real, "the control's output is neither input's result"
        if is_poison and overtook:
            print(f"side stream used for the module: {k} ({hex(side.cuda_stream)})")
            return side, delay, k
    pytest.fail(f"on none of {MAX_STREAMS} side streams did work queued on the null stream overtake the delay: {seen}; these tests would pass blind")


def _run(row, host: dict, dev: str, gpu_device: int):
    """The warm call on the default stream: (outputs on the host, host seconds of call + wait)."""
    import torch
    ctx = SC.Ctx(gpu_device)
    try:
        if row.prepare:
            row.prepare(ctx, host)
        bufs = _upload(row, host, dev)
        torch.cuda.synchronize(gpu_device)
        t0 = time.perf_counter()
        out = row.call(bufs, ctx)
        torch.cuda.synchronize(gpu_device)
        t_call = time.perf_counter() - t0
        got = _fetch(out)
        torch.cuda.synchronize(gpu_device)
        assert ctx.guards_intact(), f"{row.key}: a canary around an output is gone (default stream)"
        return got, t_call
    finally:
        ctx.close()


@pytest.mark.parametrize("row", SC.all_rows(), ids=str)
def test_entry_on_a_side_stream(row, instrument, gpu_device):
    with _latched():
        _entry_on_a_side_stream(row, instrument, gpu_device)


def _entry_on_a_side_stream(row, instrument, gpu_device):
    import torch
    side, delay, k = instrument
    dev = f"cuda:{gpu_device}"
    real, poison = SC.case(row.key, "real"), SC.case(row.key, "poison")
    want = list(SC.want(row.key, "real"))

    # 1. the warm call, default stream, real input
    got, t_call = _run(row, real, dev, gpu_device)
    row.same(got, want)
    ms = max(FACTOR * 1000.0 * t_call, FLOOR_MS)
    assert ms <= CEILING_MS, f"{row.key}: the warm call took {1000 * t_call:.1f} ms, its delay would be {ms:.0f} ms: the row's case is too large"

    # 2. the side stream: poison in the input buffers; delay, copies of the real input, the entry
    ctx = SC.Ctx(gpu_device)
    try:
        if row.prepare:
            row.prepare(ctx, real)
        bufs, src = _upload(row, poison, dev), _upload(row, real, dev)
        for name in row.host_inputs:
            bufs[name] = src[name]
        torch.cuda.synchronize(gpu_device)
        with torch.cuda.stream(side):
            e0, e1 = delay.queue(ms)
            for name in _device_names(row, real):
                bufs[name].copy_(src[name])
            out = row.call(bufs, ctx)
            running = not e1.query()                                              # the clock: was the delay still spinning when the call came back?
            got = _fetch(out)                                                     # (what came back in host memory is taken as it is: no wait of ours)
            back = {name: bufs[name].cpu().numpy() for name in _device_names(row, real) if name not in row.inout}
        side.synchronize()
        measured = e0.elapsed_time(e1)
        print(f"{row.key} ({row.layer}, {row.contract}): t_call {1000 * t_call:.3f} ms, delay asked {ms:.1f} ms, measured {measured:.1f} ms, side stream {k} "
              f"({hex(side.cuda_stream)}); the call returned {'while the delay ran' if running else 'after the delay'}")
        assert measured >= ms, (measured, ms)
        if row.contract == "async":
            assert running, f"{row.key} is asynchronous by its header, but the call waited for the stream or the device ({measured:.0f} ms of delay were over)"
        else:
            assert not running, f"{row.key} is synchronous by its header, but it returned while the work in front of it was still running"
        row.same(got, want)                                                       # the host model's result for the REAL input
        assert ctx.guards_intact(), f"{row.key}: a canary around an output is gone"
        for name, a in back.items():
            assert np.array_equal(a, real[name]), f"{row.key}: the input {name} was changed"
    finally:
        torch.cuda.synchronize(gpu_device)
        ctx.close()


# ------------------------------------------------------------------------------------------------------------ the on-device chains
def _chain(run, real: np.ndarray, poison: np.ndarray, instrument, gpu_device):
    """``run(device tensor)`` on the default stream, then on the side stream behind the delay with the poison in the buffer first."""
    with _latched():
        return _chain_latched(run, real, poison, instrument, gpu_device)


def _chain_latched(run, real, poison, instrument, gpu_device):
    import torch
    side, delay, k = instrument
    dev = f"cuda:{gpu_device}"
    t0 = time.perf_counter()
    first = run(_up(real, dev))
    torch.cuda.synchronize(gpu_device)
    t_call = time.perf_counter() - t0
    ms = max(FACTOR * 1000.0 * t_call, FLOOR_MS)
    assert ms <= CEILING_MS, (t_call, ms)
    buf, src = _up(poison, dev), _up(real, dev)
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.stream(side):
        e0, e1 = delay.queue(ms)
        buf.copy_(src)
        second = run(buf)
    side.synchronize()
    print(f"t_call {1000 * t_call:.3f} ms, delay asked {ms:.1f} ms, measured {e0.elapsed_time(e1):.1f} ms, side stream {k}")
    assert e0.elapsed_time(e1) >= ms
    assert np.array_equal(buf.cpu().numpy(), real)
    return first, second


def test_soft_to_vcdu_on_a_side_stream(instrument, gpu_device):
    """The 5-frame Reed-Solomon stream at 3 dB, one hypothesis, through rs.soft_to_vcdu: on the side stream what it gives on the default
    stream, and the VCDUs that were sent."""
    import frames_util as U
    import rs_util as R
    from meteor_demod_amd import rs
    st = R.stream()
    real = st.received(0, 3.0, seed=300)

    def run(soft):
        vcdu, info, found = rs.soft_to_vcdu(soft)
        return vcdu.cpu().numpy(), info.cpu().numpy(), found
    first, second = _chain(run, real, U.noise(len(real), seed=9), instrument, gpu_device)
    for vcdu, info, found in (first, second):
        assert len(found) >= 1 and all(f.position in st.positions and f.hypothesis == 0 for f in found)
        for j, f in enumerate(found):
            assert bytes(vcdu[j]) == bytes(st.vcdus[st.positions.index(f.position)]), j
        assert not info[:, 4:].any()
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and first[2] == second[2]


def test_soft_to_image_on_a_side_stream(instrument, gpu_device):
    """The one-strip-row picture at 3 dB through image.soft_to_image: on the side stream what it gives on the default stream, and the
    picture that was sent."""
    import frames_util as U
    import image_util as I
    from meteor_demod_amd import image
    _, packets, _ = I.sent()
    st = I.stream()
    real = st.received(2, 3.0, seed=77)
    want = I.expected_picture(packets, I.PIC_ROWS)
    first, second = _chain(lambda soft: image.soft_to_image(soft), real, U.noise(len(real), seed=10), instrument, gpu_device)
    for res, found in (first, second):
        assert len(found) >= st.n_frames - I.TAIL_IDLE and res.summary["placed"] == 42 and res.summary["rows"] == I.PIC_ROWS
        for j, a in enumerate((64, 65, 66)):
            assert np.array_equal(res.images[a], want[j]) and res.filled[a].all()
    assert first[1] == second[1] and np.array_equal(first[0].strips, second[0].strips) and np.array_equal(first[0].desc, second[0].desc)
