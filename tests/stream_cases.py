"""The table of device entries: one row per exported function that takes a ``hip_stream`` (include/*.h), for the tests of the stream
contract - tests/test_stream_cases_host.py (the table is complete; a row's poison is not its real input) and
tests/test_gpu_streams.py (every entry on a side stream behind a delay, against the host model).

A row holds the header's word for the entry (``async``: queued, the call returns at once; ``sync``: the call waits for the stream),
the smallest existing case of its layer as ``inputs("real")``, an equally valid second input of the same shape as
``inputs("poison")``, the entry itself as ``call`` - through the Python wrapper where that one launches without waiting, through ctypes
otherwise, always on the current torch stream - and ``expected``: the host model's (the oracle's, the float64 model's) result for an
input.  Nothing here comes from a GPU run.  Where a row goes through the wrapper, the wrapper with the entry inside is what is judged: a
``sync`` row's wait may be the entry's or a read-back of the wrapper's own (frames.decode, interleave.decode, survey.*,
demodulate_recording_native); that such an entry's results are complete when it returns is what the row shows.

``call(dev, ctx)`` gets the inputs as device tensors and returns the outputs in the order of ``expected``: a device tensor is an
output in device memory, a zero-argument callable is evaluated once the test has looked at the clock (a status read-back, which
waits), anything else is what the call handed back in host memory.  ``prepare(ctx, host_inputs)`` builds what has to exist before the
delay is queued (a demodulator context), ``ctx.guarded`` makes an output between canaries."""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import Callable

import numpy as np

CANARY = 0xA5
PAD = 256                                 # canary bytes on either side of a guarded output


# ------------------------------------------------------------------------------------------------------------------ the pieces
class Ctx:
    """What one run of a row's ``call`` may use: the device, a place for ``prepare`` to leave things, guarded outputs."""

    def __init__(self, device: int):
        self.device, self.state, self.guards, self.closers = device, {}, [], []

    def guarded(self, shape, dtype):
        """A tensor of ``shape`` between two canaries (filled on the current stream)."""
        import torch
        size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        room = (size + 15) // 16 * 16
        whole = torch.full((PAD + room + PAD,), CANARY, dtype=torch.uint8, device=f"cuda:{self.device}")
        self.guards.append((whole, size))
        return whole[PAD: PAD + size].view(dtype).view(*shape)

    def guards_intact(self) -> bool:
        for whole, size in self.guards:
            a = whole.cpu().numpy()
            if not ((a[:PAD] == CANARY).all() and (a[PAD + (size + 15) // 16 * 16:] == CANARY).all()):
                return False
        return True

    def close(self) -> None:
        for f in reversed(self.closers):
            f()
        self.closers, self.state, self.guards = [], {}, []


def exact(got: list, want: list) -> None:
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (k, int((g != w).sum()), "elements differ")


def differs_exact(a: list, b: list) -> bool:
    """Every output of a differs from the same output of b."""
    return all(np.asarray(x).shape != np.asarray(y).shape or not np.array_equal(x, y) for x, y in zip(a, b))


@dataclass
class Row:
    function: str
    layer: str
    contract: str                                   # "async" or "sync": the header's word
    inputs: Callable[[str], dict]                   # "real" / "poison" -> {name: numpy array}
    expected: Callable[[dict], list]
    call: Callable[[dict, Ctx], list]
    same: Callable[[list, list], None] = exact      # got, want: raises when they are not the same under the layer's bar
    differs: Callable[[list, list], bool] = differs_exact
    prepare: Callable[[Ctx, dict], None] | None = None
    inout: tuple = ()                               # inputs the entry writes (they are outputs as well)
    host_inputs: tuple = ()                         # inputs that stay in host memory (the entry takes them there)
    case: str = ""                                  # a name, for a second case of a function beside its row of the table

    @property
    def key(self) -> str:
        return f"{self.function}[{self.case}]" if self.case else self.function

    def __str__(self):
        return self.key


def _cached(f):
    return functools.lru_cache(maxsize=None)(f)


def _stream(device: int = 0) -> C.c_void_p:
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check(code: int, what: str) -> int:
    from meteor_demod_amd._capi import check
    return check(code, what)


def _i32(a) -> np.ndarray:
    """The words of a uint32 array as int32 (torch has no uint32 arithmetic; the entries take the words)."""
    return np.ascontiguousarray(a).view(np.int32)


# ======================================================================================================== demodulator (main header)
N_STREAMS, N_SAMPLES, PITCH, HALF = 70, 2000, 640, 1000
PICKS = (0, 1, 63, 64, 69)                                   # the streams whose state is read or written one by one
LOCK_SAMPLES = 16000                                         # long enough for the carrier loop to lock (the lock-event row)


def _cfg1():
    from meteor_demod_amd import DemodConfig
    return DemodConfig(samplerate=230000)                    # BASELINE configs[1]


@_cached
def _iq(which: str, n: int = N_SAMPLES) -> np.ndarray:
    """int16 [70, n, 2]: 70 synthetic QPSK streams, each with its own seed and carrier offset."""
    from meteor_demod_amd import synth
    cfg, base = _cfg1(), {"real": 10, "poison": 5000}[which]
    return np.stack([synth.generate_host(synth.make_stream(base + i, cfg.samplerate, cfg.symrate, f0_hz=150.0 * i, esn0_db=18.0), n)
                     for i in range(N_STREAMS)])


def _key(iq: np.ndarray):
    return (iq.shape, hash(iq.tobytes()))


_ORACLE = {}


def _oracle(iq: np.ndarray, streams=None, cut: int = 0):
    """Per stream of ``streams``: (soft, lock events, state after, history after) of the oracle on iq[s] - with ``cut`` the oracle
    runs iq[s][:cut] first and what comes back is the second piece's soft and the state between the pieces."""
    import oracle_py as O
    import demod_instances as M
    streams = tuple(range(iq.shape[0])) if streams is None else tuple(streams)
    k = (_key(iq), streams, cut)
    if k not in _ORACLE:
        out = {}
        for s in streams:
            ost = O.OracleStream(_cfg1())
            if cut:
                ost.run(iq[s][:cut])
                mid, mid_hist = M._snapshot(ost), ost.history()
                soft, _, ev = ost.run(iq[s][cut:])
                out[s] = (soft, ev, mid, mid_hist)
            else:
                soft, _, ev = ost.run(iq[s])
                out[s] = (soft, ev, M._snapshot(ost), ost.history())
        _ORACLE[k] = out
    return _ORACLE[k]


def _padded(softs, pitch: int, rows: int | None = None, first: int = 0):
    """(int8 [rows, pitch, 2] with row first + s = the first min(count, pitch) symbols of stream s, int64 counts)."""
    n = len(softs)
    out = np.zeros((rows if rows is not None else n, pitch, 2), dtype=np.int8)
    for s, soft in enumerate(softs):
        k = min(len(soft), pitch)
        out[first + s, :k] = soft[:k]
    return out, np.array([len(x) for x in softs], dtype=np.int64)


def _soft_same(got: list, want: list) -> None:
    """(soft rows, counts): the counts are equal and every row is equal as far as its count reaches (behind it a row is not written)."""
    g_soft, g_cnt = np.asarray(got[0]), np.asarray(got[1]).astype(np.int64).reshape(-1)
    w_soft, w_cnt = want
    assert np.array_equal(g_cnt, w_cnt), (g_cnt.tolist()[:8], w_cnt.tolist()[:8])
    first = (g_soft.shape[0] - len(w_cnt)) // 2 if g_soft.shape[0] != len(w_cnt) else 0
    for s, n in enumerate(w_cnt):
        k = min(int(n), w_soft.shape[1], g_soft.shape[1])
        assert np.array_equal(g_soft[first + s, :k], w_soft[first + s, :k]), (s, k)


def _soft_differs(a: list, b: list) -> bool:
    """Every stream's symbols differ.  The counts, which the GPU test compares as well, cannot tell two inputs apart: a stream's count
    follows from its length and the symbol rate (626 symbols of 2000 samples at 72 k in 230 kS/s, whatever the seed), and the symbol
    clock holds its word within 1 / 4096 of the nominal rate; an entry that read the poison is caught by its symbols."""
    k = int(min(a[1].min(), b[1].min(), a[0].shape[1]))
    return all(not np.array_equal(x[:k], y[:k]) for x, y in zip(a[0], b[0]) if x.any() or y.any())


def _demod(ctx: Ctx, n_streams: int = N_STREAMS):
    from meteor_demod_amd import Demodulator
    d = Demodulator(_cfg1(), n_streams, ctx.device)
    ctx.closers.append(d.close)
    ctx.state["d"] = d
    return d


def _prepare_demod(ctx: Ctx, host: dict) -> None:
    _demod(ctx)


def _counts(d):
    return lambda: np.array([s.symbols_this_call for s in d.status()], dtype=np.int64)


def _demod_inputs(which: str) -> dict:
    return {"iq": _iq(which)}


def _expect_soft(pitch_of=lambda n: n + 8):
    def f(inp):
        o = _oracle(inp["iq"])
        soft, cnt = _padded([o[s][0] for s in range(N_STREAMS)], pitch_of(inp["iq"].shape[1]))
        return [soft, cnt]
    return f


def _call_uniform(dev, ctx):
    d = ctx.state["d"]
    return [d.process(dev["iq"]), _counts(d)]


# the ragged form: stream s takes N_SAMPLES - 7 s samples from an odd offset of one flat buffer
RAGGED_COUNTS = np.array([N_SAMPLES - 7 * s for s in range(N_STREAMS)], dtype=np.int32)
RAGGED_OFFSETS = (3 + np.concatenate([[0], np.cumsum(RAGGED_COUNTS[:-1] + 1)])).astype(np.int64)


def _ragged_inputs(which: str) -> dict:
    iq = _iq(which)
    flat = np.zeros((int(RAGGED_OFFSETS[-1] + RAGGED_COUNTS[-1]) + 64, 2), dtype=np.int16)
    for s in range(N_STREAMS):
        flat[RAGGED_OFFSETS[s]: RAGGED_OFFSETS[s] + RAGGED_COUNTS[s]] = iq[s, : RAGGED_COUNTS[s]]
    return {"iq_flat": flat, "offsets": RAGGED_OFFSETS.copy(), "counts": RAGGED_COUNTS.copy()}


def _ragged_expected(inp):
    import oracle_py as O
    k = ("ragged", _key(inp["iq_flat"]))
    if k not in _ORACLE:
        softs = [O.oracle_demod(_cfg1(), inp["iq_flat"][inp["offsets"][s]: inp["offsets"][s] + inp["counts"][s]])[0] for s in range(N_STREAMS)]
        _ORACLE[k] = _padded(softs, N_SAMPLES + 8)
    return list(_ORACLE[k])


def _call_ragged(dev, ctx):
    import torch
    d = ctx.state["d"]
    soft = torch.empty((N_STREAMS, N_SAMPLES + 8, 2), dtype=torch.int8, device=dev["iq_flat"].device)
    d.process_ragged(dev["iq_flat"], dev["offsets"], dev["counts"], soft)
    return [soft, _counts(d)]


def _prepare_dirty(ctx: Ctx, host: dict) -> None:
    """A context that has already run: a reset that did not happen, or happened out of turn, shows."""
    import torch
    d = _demod(ctx)
    d.process(torch.from_numpy(np.array(_iq("poison"))).to(f"cuda:{ctx.device}"))
    torch.cuda.synchronize(ctx.device)


def _call_reset(dev, ctx):
    d = ctx.state["d"]
    d.process(dev["iq"])                                    # (more dirt, on the same stream: the reset has to come behind it)
    d.reset()
    return [d.process(dev["iq"]), _counts(d)]


def _call_compact(dev, ctx):
    d = ctx.state["d"]
    soft = d.process(dev["iq"])
    out = ctx.guarded((N_STREAMS, PITCH, 2), soft.dtype)
    d.compact(soft, PITCH, out=out)
    return [out, _counts(d)]


def _fanin_expected(inp):
    o = _oracle(inp["iq"])
    soft, cnt = _padded([o[s][0] for s in range(N_STREAMS)], PITCH, rows=N_STREAMS + 2, first=1)
    return [soft, cnt]


def _call_fanin(dev, ctx):
    import torch
    d = ctx.state["d"]
    soft = d.process(dev["iq"])
    dst = ctx.guarded((N_STREAMS + 2, PITCH, 2), torch.int8)
    counts = ctx.guarded((N_STREAMS + 2,), torch.int32)
    d.fanin_peer(soft, PITCH, dst, 1, counts)
    return [dst, lambda: counts[1: 1 + N_STREAMS].cpu().numpy().astype(np.int64)]


STATUS_FIELDS = ("n_samples", "n_symbols", "first_lock_symbol", "symbols_this_call", "lock_events_this_call", "pll_freq", "omega", "gain", "locked",
                 "locked_once", "overflow")


def _status_expected(inp):
    o = _oracle(inp["iq"])
    rows = []
    for s in range(N_STREAMS):
        soft, ev, st, _ = o[s]
        rows.append((st["n_samples"], st["n_symbols"], st["first_lock_symbol"], len(soft), len(ev), st["pll_freq"], st["t_freq"], st["gain"], st["locked"],
                     st["locked_once"], 0))
    return [np.array(rows, dtype=np.float64)]


def _call_status(dev, ctx):
    d = ctx.state["d"]
    d.process(dev["iq"])
    return [np.array([[getattr(s, f) for f in STATUS_FIELDS] for s in d.status()], dtype=np.float64)]


def _lock_inputs(which: str) -> dict:
    return {"iq": _iq(which, LOCK_SAMPLES)}


def _events(o) -> np.ndarray:
    return np.array([(s, e[0], e[1]) for s in PICKS for e in o[s][1]], dtype=np.int64).reshape(-1, 3)


def _lock_expected(inp):
    return [_events(_oracle(inp["iq"], PICKS))]


def _call_lock_events(dev, ctx):
    d = ctx.state["d"]
    d.process(dev["iq"])
    return [np.array([(s, e[0], e[1]) for s in PICKS for e in d.lock_events(s)], dtype=np.int64).reshape(-1, 3)]


STATE_PAIRS = (("agc_gain", "gain"), ("agc_bias_re", "bias_re"), ("agc_bias_im", "bias_im"), ("pll_phase", "pll_phase"), ("pll_freq", "pll_freq"),
               ("pll_err", "pll_err"), ("t_phase", "t_phase"), ("t_freq", "t_freq"), ("t_prev", "t_prev"), ("oqpsk_inphase", "inphase"),
               ("pll_locked", "locked"), ("pll_locked_once", "locked_once"), ("pll_updown", "updown"), ("t_dual_state", "dual_state"),
               ("n_samples", "n_samples"), ("n_symbols", "n_symbols"), ("first_lock_symbol", "first_lock_symbol"))


def _state_expected(inp):
    o = _oracle(inp["iq"], PICKS)
    return [np.array([[o[s][2][b] for _, b in STATE_PAIRS] for s in PICKS], dtype=np.float64)]


def _call_get_state(dev, ctx):
    d = ctx.state["d"]
    d.process(dev["iq"])
    return [np.array([[getattr(d.get_state(s), a) for a, _ in STATE_PAIRS] for s in PICKS], dtype=np.float64)]


def _history_expected(inp):
    o, taps = _oracle(inp["iq"], PICKS), _cfg1().taps
    return [np.stack([o[s][3][-(taps - 1):] for s in PICKS]).astype(np.float32)]


def _call_get_history(dev, ctx):
    d, taps = ctx.state["d"], _cfg1().taps
    d.process(dev["iq"])
    return [np.stack([d.get_history(s)[-(taps - 1):] for s in PICKS]).astype(np.float32)]


def _seeded_expected(inp):
    """The second half of the picked streams, demodulated from the oracle's state and history after the first half."""
    o = _oracle(inp["iq"], PICKS, cut=HALF)
    soft, cnt = _padded([o[s][0] for s in PICKS], N_SAMPLES - HALF + 8)
    return [soft, cnt]


def _call_seeded(history_first: bool):
    """Both setters behind a call that leaves another state: mdemod_set_state and mdemod_set_history of the picked streams from the
    oracle's run of the first half (the host's copy of the input in ctx), then the second half.  The row's own setter comes first: it
    is the one queued directly behind the delayed process call (the first setter's wait drains the stream for all that follow)."""
    def call(dev, ctx):
        return _seeded(dev, ctx, history_first)
    return call


def _seeded(dev, ctx, history_first: bool):
    import demod_instances as M
    d = ctx.state["d"]
    iq = ctx.state["host"]["iq"]
    o = _oracle(iq, PICKS, cut=HALF)
    d.process(dev["iq"])                                     # every stream somewhere else, on the same stream
    hpad = d.history_len()
    for s in PICKS:
        if history_first:
            d.set_history(s, M.decode(iq[s][HALF - hpad: HALF]))
            d.set_state(s, M.to_stream_state(o[s][2]))
        else:
            d.set_state(s, M.to_stream_state(o[s][2]))
            d.set_history(s, M.decode(iq[s][HALF - hpad: HALF]))
    soft = d.process(dev["iq"][:, HALF:])
    picks = list(PICKS)
    return [lambda: soft[picks].cpu().numpy(), lambda: np.array([d.status(s, 1)[0].symbols_this_call for s in PICKS], dtype=np.int64)]


def _prepare_seeded(ctx: Ctx, host: dict) -> None:
    _demod(ctx)
    ctx.state["host"] = host


# ---- one recording: short enough that the serial head never hands over, so every symbol is the oracle's
REC_SAMPLES = 8000


def _rec_inputs(which: str) -> dict:
    from meteor_demod_amd import synth
    st = synth.make_stream({"real": 3, "poison": 4}[which], 230000, 72000, f0_hz=0.0)
    return {"iq": synth.generate_host(st, REC_SAMPLES)}


def _rec_expected(inp):
    import oracle_py as O
    soft = O.oracle_demod(_cfg1(), inp["iq"])[0]
    return [soft]


def _call_recording(dev, ctx):
    import torch
    from meteor_demod_amd.recording import demodulate_recording_native
    cap = REC_SAMPLES + 64
    out = ctx.guarded((cap, 2), torch.int8)
    soft, rep = demodulate_recording_native(_cfg1(), dev["iq"], pilot_margin_symbols=160000, device=ctx.device, soft=out)
    assert rep.n_tiles == 0                                  # (all serial: what makes the oracle the expectation)
    return [soft]


# ---- the stitcher's setters (csrc/mdemod_internal_api.h): first half, the setter from a device array, second half; the oracle runs
# the first half, takes the same change in its state, and runs the second half
def _centre() -> np.float32:
    import oracle_py as O
    return np.float32(O.OracleStream(_cfg1()).consts.t_center)


def _seed_inputs(which: str) -> dict:
    """The input and, per stream, every setter's array (each row uses its own): other values for the poison."""
    k = np.arange(N_STREAMS) + (0 if which == "real" else 1)
    return {"iq": _iq(which),
            "turns": (k % 7 - 2).astype(np.int32),                                            # -2 .. 4: every residue of 4, negative ones too
            "freq": (0.004 * (k % 9 - 4)).astype(np.float32), "updown": np.where(k % 3 == 0, -1, 1).astype(np.int32),
            "gain": np.where(k % 11 == 5, -1.0, 0.05 + 0.01 * k).astype(np.float32),          # (a negative seed becomes 0, agc.c:23)
            "t_freq": (np.float64(_centre()) * (1.0 + (k % 9 - 4) / 40000.0)).astype(np.float32)}      # inside centre +- centre / 4096: taken as it is


def _set_rotate(st, inp, s):
    import math
    k = int(inp["turns"][s]) & 3
    if k:
        st.pll_phase = float(np.float32(math.fmod(float(st.pll_phase) + k * (math.pi / 2), 2 * math.pi)))


def _set_carrier(st, inp, s):
    st.pll_freq, st.updown = float(inp["freq"][s]), (1 if inp["updown"][s] > 0 else -1)


def _set_gain(st, inp, s):
    st.gain = max(float(inp["gain"][s]), 0.0)


def _set_clock(st, inp, s):
    st.t_freq = float(inp["t_freq"][s])


def _halves_expected(change):
    def expected(inp):
        import oracle_py as O
        softs = []
        for s in range(N_STREAMS):
            ost = O.OracleStream(_cfg1())
            ost.run(inp["iq"][s][:HALF])
            change(ost.state, inp, s)
            softs.append(ost.run(inp["iq"][s][HALF:])[0])
        return list(_padded(softs, N_SAMPLES - HALF + 8))
    return expected


def _call_halves(setter):
    def call(dev, ctx):
        d = ctx.state["d"]
        d.process(dev["iq"][:, :HALF])
        setter(d, dev)                                       # queued behind the first half, in front of the second
        return [d.process(dev["iq"][:, HALF:]), _counts(d)]
    return call


def _internal_rows() -> list:
    L = "demodulator (internal)"
    each = ((("mdemod_rotate_carrier"), _set_rotate, lambda d, dev: d.rotate_carrier(dev["turns"])),
            (("mdemod_set_carrier_seeds"), _set_carrier, lambda d, dev: d.set_carrier_seeds(dev["freq"], dev["updown"])),
            (("mdemod_set_gain_seeds"), _set_gain, lambda d, dev: d.set_gain_seeds(dev["gain"])),
            (("mdemod_set_clock_seeds"), _set_clock, lambda d, dev: d.set_clock_seeds(dev["t_freq"])))
    return [Row(name, L, "async", _seed_inputs, _halves_expected(change), _call_halves(setter), _soft_same, _soft_differs, _prepare_demod)
            for name, change, setter in each]


def _demod_rows() -> list:
    L = "demodulator"
    return [
        Row("mdemod_process_device_uniform", L, "async", _demod_inputs, _expect_soft(), _call_uniform, _soft_same, _soft_differs, _prepare_demod),
        Row("mdemod_process_device", L, "async", _ragged_inputs, _ragged_expected, _call_ragged, _soft_same, _soft_differs, _prepare_demod),
        Row("mdemod_reset", L, "async", _demod_inputs, _expect_soft(), _call_reset, _soft_same, _soft_differs, _prepare_dirty),
        Row("mdemod_compact_soft", L, "async", _demod_inputs, _expect_soft(lambda n: PITCH), _call_compact, _soft_same, _soft_differs, _prepare_demod),
        Row("mdemod_fanin_peer", L, "async", _demod_inputs, _fanin_expected, _call_fanin, _soft_same,
            lambda a, b: _soft_differs([a[0][1:-1], a[1]], [b[0][1:-1], b[1]]), _prepare_demod),
        Row("mdemod_get_status", L, "sync", _demod_inputs, _status_expected, _call_status, prepare=_prepare_demod),
        Row("mdemod_get_lock_events", L, "sync", _lock_inputs, _lock_expected, _call_lock_events, prepare=_prepare_demod),
        Row("mdemod_get_state", L, "sync", _demod_inputs, _state_expected, _call_get_state, prepare=_prepare_demod),
        Row("mdemod_set_state", L, "sync", _demod_inputs, _seeded_expected, _call_seeded(False), _soft_same, _soft_differs, _prepare_seeded),
        Row("mdemod_get_history", L, "sync", _demod_inputs, _history_expected, _call_get_history, prepare=_prepare_demod),
        Row("mdemod_set_history", L, "sync", _demod_inputs, _seeded_expected, _call_seeded(True), _soft_same, _soft_differs, _prepare_seeded),
        Row("mdemod_demodulate_recording", L, "sync", _rec_inputs, _rec_expected, _call_recording),
    ]


# ========================================================================================================================= front end
FE_N, FE_D, FE_FS, FE_OFFSET = 4003, 8, 2000000, 312500.0


def _fe_cfgs():
    from meteor_demod_amd import DemodConfig, FrontEndConfig
    return DemodConfig(samplerate=FE_FS, bps=16), FrontEndConfig(FE_OFFSET, FE_D)


def _fe_inputs(which: str) -> dict:
    rng = np.random.default_rng({"real": 816, "poison": 817}[which])
    return {"iq": np.clip(rng.normal(0, 3000, size=(FE_N, 2)), -32768, 32767).astype(np.int16)}


def _fe_model(x: np.ndarray) -> np.ndarray:
    """float64: the library's phase words (full 32 bits) and float taps, zero history (the model of tests/test_gpu_frontend.py)."""
    from meteor_demod_amd import design_taps
    from meteor_demod_amd.frontend import phase_step
    cfg, fe = _fe_cfgs()
    h, _ = design_taps(cfg, fe)
    xc = x.astype(np.float64)
    z = xc[:, 0] + 1j * xc[:, 1]
    n = np.arange(len(z), dtype=np.uint64)
    p = (n * np.uint64(phase_step(FE_OFFSET, FE_FS))) & np.uint64(0xFFFFFFFF)
    z = z * np.exp(2j * np.pi * p.astype(np.float64) / 2.0 ** 32)
    return np.convolve(z, h.astype(np.float64))[: len(z)][::FE_D]


def _fe_rms(x) -> float:
    return float(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1).mean()))


def _fe_expected(inp):
    return [_fe_model(inp["iq"]), np.array([-(-FE_N // FE_D)], dtype=np.int64), np.float64(_fe_rms(inp["iq"]))]


def _fe_same(got, want):
    """The existing bar of the front end: max |error| <= 1e-4 of the input's RMS, and exactly ceil(n / D) outputs."""
    y, n, rms = want
    cnt = np.asarray(got[1]).astype(np.int64).reshape(-1)
    assert np.array_equal(cnt, n), (cnt, n)
    g = np.asarray(got[0]).astype(np.float64)[0, : int(n[0])]
    err = np.abs((g[:, 0] + 1j * g[:, 1]) - y).max()
    assert err <= 1e-4 * rms, err / rms


def _fe_differs(a, b) -> bool:
    return bool(np.abs(a[0] - b[0]).max() > 1e-2 * max(a[2], b[2]))


def _prepare_fe(cfgs, first_launch: bool = False):
    """``first_launch``: the demodulator's f32 instance is launched once on 8 samples by a front end of its own before anything is
    timed (the runtime loads a kernel at its first launch: 50 ms for this one, which would pass for the call's own time and ask for
    a delay of a second)."""
    def prepare(ctx: Ctx, host: dict) -> None:
        import torch
        from meteor_demod_amd import FrontEnd
        cfg, fe = cfgs()
        if first_launch:
            with FrontEnd(cfg, fe, 1, device=ctx.device) as once:
                once.process(torch.zeros((1, 8, 2), dtype=torch.int16, device=f"cuda:{ctx.device}"))
                torch.cuda.synchronize(ctx.device)
        f = FrontEnd(cfg, fe, 1, device=ctx.device)
        ctx.closers.append(f.close)
        ctx.state["f"] = f
    return prepare


def _call_baseband(dev, ctx):
    import torch
    f, iq = ctx.state["f"], dev["iq"]
    off = torch.zeros(1, dtype=torch.int64, device=iq.device)
    cnt = torch.full((1,), FE_N, dtype=torch.int32, device=iq.device)
    bb, n_out = f.baseband_ragged(iq, off, cnt, FE_N)
    return [bb, n_out]


# front end + demodulator: the identity front end (D 1, offset 0) hands the converted samples on, and the demodulator's symbols
# on them are the oracle's (tests/test_gpu_frontend.py::test_identity_front_end_gives_the_references_bytes)
FEP_N = 4000


def _fep_cfgs():
    from meteor_demod_amd import DemodConfig, FrontEndConfig
    return DemodConfig(samplerate=230000, bps=16), FrontEndConfig(0.0, 1)


def _fep_inputs(which: str) -> dict:
    return {"iq": np.ascontiguousarray(_iq(which)[3:5].reshape(-1, 2))[:FEP_N]}


def _fep_expected(inp):
    import oracle_py as O
    from meteor_demod_amd.frontend import output_config
    soft = O.oracle_demod(output_config(*_fep_cfgs()), inp["iq"].astype(np.float32))[0]
    out, cnt = _padded([soft], FEP_N + 16)
    return [out, cnt]


def _fe_counts(f):
    return lambda: np.array([f.status()[0].symbols_this_call], dtype=np.int64)


def _call_fe_process(dev, ctx):
    f = ctx.state["f"]
    return [f.process(dev["iq"].reshape(1, FEP_N, 2)), _fe_counts(f)]


def _call_fe_reset(dev, ctx):
    f = ctx.state["f"]
    f.process(dev["iq"].reshape(1, FEP_N, 2))
    f.reset()
    return [f.process(dev["iq"].reshape(1, FEP_N, 2)), _fe_counts(f)]


def _fe_rows() -> list:
    L = "front end"
    return [
        Row("mdemod_fe_baseband_device", L, "async", _fe_inputs, _fe_expected, _call_baseband, _fe_same, _fe_differs, _prepare_fe(_fe_cfgs)),
        Row("mdemod_fe_process_device", L, "async", _fep_inputs, _fep_expected, _call_fe_process, _soft_same, _soft_differs, _prepare_fe(_fep_cfgs, True)),
        Row("mdemod_fe_reset", L, "async", _fep_inputs, _fep_expected, _call_fe_reset, _soft_same, _soft_differs, _prepare_fe(_fep_cfgs, True)),
    ]


# ============================================================================================================================ survey
SV_FFT, SV_FS, SV_N = 4096, 2400000, 1 << 18


def _sv_cfg():
    from meteor_demod_amd import DemodConfig
    return DemodConfig(samplerate=SV_FS, bps=16)


@_cached
def _sv_input(which: str) -> np.ndarray:
    """s16 [n, 2]: white noise with a band of one LRPT signal's width (72 k symbols/s, roll-off 0.6) 20 dB above it, at +301.2 kHz
    (real) or -412.5 kHz (poison)."""
    centre = {"real": 301200.0, "poison": -412500.0}[which]
    rng = np.random.default_rng(int(abs(centre)))
    w = rng.normal(size=SV_N) + 1j * rng.normal(size=SV_N)
    f = np.fft.fftfreq(SV_N, 1.0 / SV_FS)
    band = np.fft.ifft(np.fft.fft(rng.normal(size=SV_N) + 1j * rng.normal(size=SV_N)) * (np.abs(f - centre) <= 36000.0 * 1.3))
    band *= 10.0 * np.sqrt(SV_N / max(int((np.abs(f - centre) <= 36000.0 * 1.3).sum()), 1))
    z = 300.0 * (w + band * np.exp(0j))
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)), -32768, 32767).astype(np.int16)


def _sv_inputs(which: str) -> dict:
    return {"iq": _sv_input(which)}


def _spectrum_inputs(which: str) -> dict:
    return {"iq": _sv_input(which)[: 8 * SV_FFT + SV_FFT // 3 + 1]}


def _spectrum_expected(inp):
    import survey_util as SU
    return [SU.model64(inp["iq"], 16, SV_FFT, 1)]


def _spectrum_same(got, want):
    """The existing bar of the spectrum: |got / want - 1| <= 1e-5 at every bin."""
    g = np.asarray(got[0]).astype(np.float64)
    assert g.shape == want[0].shape
    e = float(np.abs(g / want[0] - 1).max())
    assert e <= 1e-5, e


def _call_spectrum(dev, ctx):
    from meteor_demod_amd import survey
    return [survey.spectrum(_sv_cfg(), dev["iq"], fft_size=SV_FFT, rows=1)]


def _survey_expected(inp):
    """The strongest candidate of the host-only detector on the float64 model's waterfall."""
    import survey_util as SU
    from meteor_demod_amd import survey
    psd = SU.model64(inp["iq"], 16, SV_FFT, 8).astype(np.float32)
    hits = survey.detect(_sv_cfg(), psd, max_candidates=1)
    return [np.array([h.coarse_offset_hz for h in hits], dtype=np.float64)]


def _survey_same(got, want):
    """One hit, its coarse offset within a bin of the model's (the bar of tests/test_gpu_survey.py: fs / fft_size)."""
    g = np.asarray(got[0], dtype=np.float64)
    assert g.shape == want[0].shape == (1,), (g, want[0])
    assert abs(g[0] - want[0][0]) <= SV_FS / SV_FFT, (g, want[0])


def _call_survey(dev, ctx):
    from meteor_demod_amd import survey
    hits = survey.survey(_sv_cfg(), dev["iq"], fft_size=SV_FFT, max_candidates=1)
    return [np.array([h.coarse_offset_hz for h in hits], dtype=np.float64)]


def _survey_rows() -> list:
    L = "survey"
    return [
        Row("mdemod_spectrum_device", L, "sync", _spectrum_inputs, _spectrum_expected, _call_spectrum, _spectrum_same,
            lambda a, b: bool(np.abs(a[0] / b[0] - 1).max() > 1e-2)),
        Row("mdemod_survey_device", L, "sync", _sv_inputs, _survey_expected, _call_survey, _survey_same,
            lambda a, b: len(a[0]) == len(b[0]) == 1 and abs(a[0][0] - b[0][0]) > 100 * SV_FS / SV_FFT),
    ]


# ============================================================================================================ frames and frames_link
def _cand_rows(cands) -> np.ndarray:
    """Candidates as the kernel writes them: int32 [windows, 4] of position low, position high, score, hypothesis."""
    a = np.array([(c.position & 0xFFFFFFFF, c.position >> 32, c.score, c.hypothesis) for c in cands], dtype=np.int64).reshape(-1, 4)
    return a.astype(np.uint32).view(np.int32) if a.size else a.astype(np.int32)


def _frame_rows(fr) -> np.ndarray:
    return np.array([(f.position, f.hypothesis, f.score, f.flags, f.channel_errors, f.run) for f in fr], dtype=np.int64).reshape(-1, 6)


@_cached
def _frames_stream(link: bool, which: str = "real"):
    """Four frames (poison: four other frames at the same positions)."""
    import frames_util as U
    import link_util as LU
    seed = {"real": 1, "poison": 2}[which]
    return LU.LinkStream(seed=6 + seed, n_frames=4, differential=True) if link else U.Stream(seed=seed, n_frames=4)


FR_H, LINK_H = 3, 13                      # the hypotheses the streams are sent through (13 = h 5, skew 1)


def _frames_inputs(link: bool):
    def f(which: str) -> dict:
        st, seed = _frames_stream(link, which), {"real": 100, "poison": 101}[which]
        return {"soft": st.received(LINK_H if link else FR_H, 3.0, seed=seed)}
    return f


def _link_kw(link: bool) -> dict:
    return dict(differential=True, skew=True) if link else {}


def _sent(link: bool):
    from meteor_demod_amd import frames
    return [frames.Frame(p, LINK_H if link else FR_H, 0, 0, 0, 0) for p in _frames_stream(link).positions]


def _frames_rows() -> list:
    from meteor_demod_amd import frames
    rows = []
    for link in (False, True):
        kw, infix, layer = _link_kw(link), ("link_" if link else ""), ("frames_link" if link else "frames")
        rows += [
            Row(f"mdemod_frames_{infix}candidates_device", layer, "async", _frames_inputs(link),
                lambda inp, kw=kw: [_cand_rows(frames.model_candidates(inp["soft"], **kw))],
                lambda dev, ctx, kw=kw: [frames.candidates_tensor(dev["soft"], **kw)]),
            Row(f"mdemod_frames_{infix}viterbi_device", layer, "sync", _frames_inputs(link),
                lambda inp, kw=kw, link=link: (lambda r: [r[0], _frame_rows(r[1])])(frames.model_viterbi(inp["soft"], _sent(link), **kw)),
                lambda dev, ctx, kw=kw, link=link: (lambda r: [r[0], _frame_rows(r[1])])(frames.viterbi(dev["soft"], _sent(link), **kw))),
            Row(f"mdemod_frames_{infix}decode_device", layer, "sync", _frames_inputs(link),
                lambda inp, kw=kw: (lambda r: [r[0], _frame_rows(r[1])])(frames.model_decode(inp["soft"], **kw)),
                lambda dev, ctx, kw=kw: (lambda r: [r[0], _frame_rows(r[1])])(frames.decode(dev["soft"], **kw))),
        ]
    return rows


# ======================================================================================================================== interleave
IL_M = 2                                  # branch delay of the small sender


@_cached
def _il_soft(which: str) -> np.ndarray:
    import interleave_util as IU
    seed, H = {"real": (200, 9), "poison": (300, 20)}[which]
    return IU.random_sender(seed, 3 * 64 + 9, IL_M, lead=21).received(H, 3.0, seed=seed + 1)


def _il_inputs(which: str) -> dict:
    return {"soft": _il_soft(which)}


def _seg_rows(segs) -> np.ndarray:
    return np.array([(s.first_symbol, s.marker_symbol, s.period, s.phase, s.hypothesis) for s in segs], dtype=np.int64).reshape(-1, 5)


def _il_table():
    """The segment table of the real stream (host memory: the gather takes it there), from the model's candidates."""
    from meteor_demod_amd import interleave as il
    soft = _il_soft("real")
    return il.track(il.model_candidates(soft), len(soft))


def _il_rows() -> list:
    from meteor_demod_amd import interleave as il
    L = "interleave"

    def decode_expected(inp):
        out, segs, p = il.model_decode(inp["soft"], branch_delay=IL_M)
        return [out, _seg_rows(segs)]

    def decode_call(dev, ctx):
        out, rep = il.decode(dev["soft"], branch_delay=IL_M)
        return [out, _seg_rows(rep.list)]

    return [
        Row("mdemod_il_candidates_device", L, "async", _il_inputs, lambda inp: [_cand_rows(il.model_candidates(inp["soft"]))],
            lambda dev, ctx: [il.candidates_tensor(dev["soft"])]),
        Row("mdemod_il_deinterleave_device", L, "async", _il_inputs,
            lambda inp: [il.model_deinterleave(inp["soft"], *_il_table(), branch_delay=IL_M)],
            lambda dev, ctx: [il.deinterleave(dev["soft"], *_il_table(), branch_delay=IL_M)]),
        Row("mdemod_il_decode_device", L, "sync", _il_inputs, decode_expected, decode_call),
    ]


IL_MANY, IL_MANY_PERIODS = 33, 200        # one segment more than travels as kernel arguments: the table goes through device memory


def _il_many():
    from meteor_demod_amd import interleave as il
    return [il.Segment(0, 5 + 241 * i, 6 * i, 5, (7 * i) % 24) for i in range(IL_MANY)], IL_MANY_PERIODS


def _il_extra_rows() -> list:
    """mdemod_il_deinterleave_device with more than 32 segments: synchronous by its header (the table is uploaded into a temporary)."""
    from meteor_demod_amd import interleave as il
    return [Row("mdemod_il_deinterleave_device", "interleave", "sync", _il_inputs,
                lambda inp: [il.model_deinterleave(inp["soft"], *_il_many(), branch_delay=IL_M)],
                lambda dev, ctx: [il.deinterleave(dev["soft"], *_il_many(), branch_delay=IL_M)], case="33 segments")]


# ================================================================================================================================ rs
def _rs_inputs(which: str) -> dict:
    import rs_util as R
    cadu = R.mixed_batch(5, seed={"real": 105, "poison": 106}[which])[1]
    return {"cadu": cadu if which == "real" else np.ascontiguousarray(np.roll(cadu, 2, axis=0))}        # (other loads in every place)


def _rs_rows() -> list:
    from meteor_demod_amd import rs
    return [Row("mdemod_rs_decode_device", "rs", "async", _rs_inputs, lambda inp: list(rs.model_decode(inp["cadu"])),
                lambda dev, ctx: list(rs.decode(dev["cadu"])))]


# ============================================================================================================================= image
def _find_inputs(which: str) -> dict:
    import image_util as I
    vcdu, info, _, _ = I.demux_batch(22)
    if which == "poison":                                   # the same frames, the other way round: other counters, other packets
        vcdu, info = vcdu[::-1], info[::-1]
    return {"vcdu": np.ascontiguousarray(vcdu), "info": np.ascontiguousarray(info)}


def _find_expected(inp):
    from meteor_demod_amd import image
    d = image.model_find(inp["vcdu"], inp["info"])
    out = np.zeros((image.MAX_PER_FRAME * 22, 16), dtype=np.uint8)
    out[: len(d)] = d.view(np.uint8).reshape(-1, 16)
    return [out, np.array([len(d)], dtype=np.int64)]


def _find_same(got, want):
    """The total, and the descriptors as far as it reaches (behind it the buffer is not written)."""
    n = int(np.asarray(got[1]).reshape(-1)[0])
    assert n == int(want[1][0]), (n, want[1])
    assert np.array_equal(np.asarray(got[0])[:n], want[0][:n])


def _call_find(dev, ctx):
    import torch
    from meteor_demod_amd import image
    n, cap = 22, image.MAX_PER_FRAME * 22
    desc = ctx.guarded((cap, 16), torch.uint8)
    total = ctx.guarded((1,), torch.int64)
    o = image.make_opts()
    _check(image.lib().mdemod_packets_find_device(C.byref(o), _ptr(dev["vcdu"]), _ptr(dev["info"]), n, _ptr(desc), cap, _ptr(total), ctx.device,
                                                       _stream(ctx.device)), "mdemod_packets_find_device")
    return [desc, total]


def _decode_inputs(which: str) -> dict:
    """The first 65 packets of the batch (poison: the other 65 of the same frames)."""
    import image_util as I
    from meteor_demod_amd import image
    _, vcdu, _ = I.decode_batch()
    d = image.model_find(vcdu)
    assert len(d) >= 130
    d = d[:65] if which == "real" else d[65:130]
    return {"vcdu": np.ascontiguousarray(vcdu), "desc": np.ascontiguousarray(d.view(np.uint8).reshape(-1, 16))}


def _decode_expected(inp):
    from meteor_demod_amd import image
    strips, sinfo = image.model_decode(inp["vcdu"], inp["desc"])
    return [strips, np.ascontiguousarray(sinfo).view(np.uint8).reshape(-1, 16)]


def _image_rows() -> list:
    from meteor_demod_amd import image
    return [
        Row("mdemod_packets_find_device", "image", "async", _find_inputs, _find_expected, _call_find, _find_same),
        Row("mdemod_image_decode_device", "image", "async", _decode_inputs, _decode_expected, lambda dev, ctx: list(image.decode(dev["vcdu"], dev["desc"]))),
    ]


# ================================================================================================ picture, map, mosaic (three slots)
def _slots(prefix: str, images, filled) -> dict:
    out = {}
    for s in range(3):
        out[f"{prefix}im{s}"], out[f"{prefix}fl{s}"] = images[s], filled[s]
    return out


def _of(d: dict, prefix: str):
    return [d[f"{prefix}im{s}"] for s in range(3)], [d[f"{prefix}fl{s}"] for s in range(3)]


PIC_ROWS, PIC_SELECT = 2, (2, 1, 0)


def _picture_inputs(which: str) -> dict:
    import picture_util as PU
    from meteor_demod_amd import picture
    d = _slots("", PU.pixels(PIC_ROWS, {"real": 102, "poison": 103}[which]), PU.masks("mixed", PIC_ROWS, {"real": 2, "poison": 3}[which]))
    d["luts"], d["cmap"] = PU.random_luts(2), _i32(picture.column_map())
    return d


def _picture_rows() -> list:
    from meteor_demod_amd import picture
    return [
        Row("mdemod_picture_histogram_device", "picture", "async", _picture_inputs,
            lambda inp: [_i32(picture.model_histogram(*_of(inp, "")).astype(np.uint32))],
            lambda dev, ctx: [picture.histogram(*_of(dev, ""))]),
        Row("mdemod_picture_render_device", "picture", "async", _picture_inputs,
            lambda inp: list(picture.model_render(*_of(inp, ""), PIC_SELECT, inp["luts"], inp["cmap"].view(np.uint32), valid=True)),
            lambda dev, ctx: list(picture.render(*_of(dev, ""), PIC_SELECT, dev["luts"], dev["cmap"], valid=True))),
    ]


@_cached
def _warp_case():
    import map_util as MU
    return next(c for c in MU.warp_cases() if c[0] == "half a pixel")           # 68 x 17: no multiple of 16 or of a block's tile


def _map_inputs(which: str) -> dict:
    import map_util as MU
    import picture_util as PU
    d = _slots("", PU.pixels(MU.SRC_ROWS, {"real": 41, "poison": 42}[which]), PU.masks("mixed", MU.SRC_ROWS, {"real": 3, "poison": 4}[which]))
    d["luts"], d["nodes"] = PU.random_luts(3), _warp_case()[3]
    return d


def _map_rows() -> list:
    from meteor_demod_amd import map as mp
    _, w, h, _ = _warp_case()
    return [Row("mdemod_map_warp_device", "map", "async", _map_inputs,
                lambda inp: list(mp.model_warp(*_of(inp, ""), PIC_SELECT, inp["luts"], inp["nodes"], w, h, valid=True)),
                lambda dev, ctx: list(mp.warp(*_of(dev, ""), PIC_SELECT, dev["luts"], dev["nodes"], w, h, valid=True)))]


MOS_W, MOS_H = 36, 150                    # no multiple of the tile


def _mosaic_inputs(which: str) -> dict:
    import mosaic_util as Z
    import picture_util as PU
    d = {}
    for k, (images, filled, luts, nodes) in enumerate(Z.sources("mixed", MOS_W, MOS_H, 2, 3)):
        if which == "poison":
            images, filled = PU.pixels(images[0].shape[0] // 8, 900 + k), PU.masks("mixed", images[0].shape[0] // 8, 950 + k)
        d.update(_slots(f"p{k}_", images, filled))
        d[f"p{k}_luts"], d[f"p{k}_nodes"] = luts, nodes
    return d


def _mosaic_sources(d: dict) -> list:
    return [(*_of(d, f"p{k}_"), d[f"p{k}_luts"], d[f"p{k}_nodes"]) for k in range(2)]


def _mosaic_rows() -> list:
    import mosaic_util as Z
    from meteor_demod_amd import mosaic as M
    mode = M.BLENDS["feather"]
    return [Row("mdemod_mosaic_blend_device", "mosaic", "async", _mosaic_inputs,
                lambda inp: list(Z.blend_reference(_mosaic_sources(inp), PIC_SELECT, MOS_W, MOS_H, mode)),
                lambda dev, ctx: list(M.blend(_mosaic_sources(dev), PIC_SELECT, MOS_W, MOS_H, mode, valid=True, cover=True)))]


# ============================================================================================================================= polar
@_cached
def _polar_case(which: str):
    """The "1 pass of 3 rows" node case of tests/test_gpu_polar.py (poison: the same pass on another orbit plane, on the same frame)."""
    import polar_util as PU_
    from meteor_demod_amd import polar as P
    pas, ref = PU_.polar_pass(80.0, 3, None, later=0)
    g = P.grid([pas], metres_per_pixel=8000.0)
    if which == "poison":
        pas, ref = PU_.polar_pass(80.0, 3, 157.0, later=0)
        g = P.model_nodes([pas], g.frame, metres_per_pixel=8000.0)
    return pas, ref, g


def _polar_inputs(which: str) -> dict:
    g = _polar_case(which)[2]
    return {"table": g.solvers[0].table}


def _polar_expected(inp):
    which = "real" if np.array_equal(inp["table"], _polar_case("real")[2].solvers[0].table) else "poison"
    return [_polar_case(which)[2].nodes[0]]


def _polar_same(got, want):
    """The header's rule for two solvers of one pass's nodes (tests/polar_util.py::agreement): no node breaks it, and nodes are there."""
    import polar_util as PU_
    pas, ref, _ = _polar_case("real")
    g = np.asarray(got[0])
    broken, _, _ = PU_.agreement(g, want[0], ref, pas.images[0].shape[0])
    assert broken == 0 and (~PU_.missing(g)).any(), broken


def _polar_differs(a, b) -> bool:
    import polar_util as PU_
    pas, ref, _ = _polar_case("real")
    return PU_.agreement(a[0], b[0], ref, pas.images[0].shape[0])[0] > 0


def _call_polar(dev, ctx):
    import torch
    from meteor_demod_amd import polar as P
    g = _polar_case("real")[2]
    s = P.Solver(g.solvers[0].fields, dev["table"])
    out = ctx.guarded(g.frame.nodes_shape, torch.int32)
    work = ctx.guarded((24 * s.table.shape[0],), torch.uint8)
    P.nodes_device(g.frame, [s], device=f"cuda:{ctx.device}", out=[out], work=work)
    return [out]


def _polar_rows() -> list:
    return [Row("mdemod_polar_nodes_device", "polar", "async", _polar_inputs, _polar_expected, _call_polar, _polar_same, _polar_differs,
                host_inputs=("table",))]


# =========================================================================================================================== overlay
OV_W, OV_H = 64, 48


def _overlay_styles():
    from meteor_demod_amd import overlay as O
    return [O.Style(128, 256, (255, 255, 0)), O.Style(300, 160, (20, 200, 90)), O.Style(0, 256, (1, 2, 3), True)]


@_cached
def _overlay_scene(seed: int):
    """Pieces of seeded polylines for every style, binned into tiles (the scene of tests/test_gpu_overlay.py at 64 x 48)."""
    from meteor_demod_amd import overlay as O
    rng, styles, parts = np.random.default_rng(seed), _overlay_styles(), []
    for s, st in enumerate(styles):
        lines = []
        for _ in range(3):
            n = int(rng.integers(2, 6))
            x0, y0 = int(rng.integers(0, 256 * OV_W)), int(rng.integers(0, 256 * OV_H))
            lines.append((x0 + np.cumsum(rng.integers(-6000, 6000, n)), y0 + np.cumsum(rng.integers(-6000, 6000, n))))
        lines.append(([-3000, 256 * OV_W + 3000], [int(rng.integers(0, 256 * OV_H + 1)), int(rng.integers(0, 256 * OV_H + 1))]))
        xs = [np.asarray(a, dtype=np.int64) for a, _ in lines]
        first = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).astype(np.uint32)
        pts = O.Points(np.concatenate(xs).astype(np.int32), np.concatenate([np.asarray(b, dtype=np.int64) for _, b in lines]).astype(np.int32), first)
        parts.append(O.pieces(pts, s, st.half_width, OV_W, OV_H))
    pcs = np.concatenate(parts)
    tile_first, items = O.bins(pcs, styles, OV_W, OV_H)
    return pcs, tile_first, items


def _overlay_inputs(which: str) -> dict:
    pcs, tile_first, items = _overlay_scene(451)
    rng = np.random.default_rng({"real": 7, "poison": 8}[which])
    return {"pixels": rng.integers(0, 256, (OV_H, OV_W, 3), dtype=np.uint8), "valid": (rng.integers(0, 2, (OV_H, OV_W)) * 255).astype(np.uint8),
            "pcs": np.ascontiguousarray(pcs).view(np.uint8).reshape(-1).copy(), "tile_first": _i32(tile_first), "items": _i32(items)}


def _overlay_expected(inp):
    from meteor_demod_amd import overlay as O
    return list(O.model_pieces(inp["pixels"], inp["pcs"].view(O.PIECE), _overlay_styles(), inp["valid"]))


def _call_overlay(dev, ctx):
    from meteor_demod_amd import overlay as O
    mask = O.draw_pieces(dev["pixels"], dev["pcs"], dev["tile_first"], dev["items"], _overlay_styles(), valid=dev["valid"], mask=True)
    return [dev["pixels"], mask]


def _overlay_rows() -> list:
    return [Row("mdemod_overlay_draw_device", "overlay", "async", _overlay_inputs, _overlay_expected, _call_overlay, inout=("pixels",))]


# ========================================================================================================================== equalise
EQ_W, EQ_H, EQ_TILE, EQ_PLANES = 39, 23, 16, 3


def _eq_opts():
    from meteor_demod_amd import equalise as E
    return E.options(tile=EQ_TILE, clip=3.0, amount=0.75, mode=1)


def _eq_inputs(which: str) -> dict:
    import equalise_ref as R
    return {"picture": R.picture_of("noise", EQ_W, EQ_H, EQ_PLANES, seed={"real": 0, "poison": 1}[which]),
            "valid": R.mask_of("gaps", "noise", EQ_W, EQ_H, EQ_TILE)[0]}


def _eq_need() -> int:
    from meteor_demod_amd import equalise as E
    return E.workspace(EQ_W, EQ_H, EQ_PLANES, _eq_opts())


def _eq_work(inp) -> np.ndarray:
    from meteor_demod_amd import equalise as E
    return E.model_workspace(inp["picture"], inp["valid"], _eq_opts())[: _eq_need()]


def _eq_out(inp) -> np.ndarray:
    from meteor_demod_amd import equalise as E
    return E.model_apply(inp["picture"], inp["valid"], tile=EQ_TILE, clip=3.0, amount=0.75, mode=1)


def _eq_apply_inputs(which: str) -> dict:
    """The second stage's inputs: the picture and the first stage's workspace, as the model fills it."""
    d = _eq_inputs(which)
    d["work"] = _eq_work(d)
    return d


def _call_eq(stage: str):
    def call(dev, ctx):
        import torch
        from meteor_demod_amd import equalise as E
        lib, o, need, st, d = E.lib(), _eq_opts(), _eq_need(), _stream(ctx.device), ctx.device
        pic, val = dev["picture"], dev["valid"]
        if stage == "tables":
            work = ctx.guarded((need,), torch.uint8)
            _check(lib.mdemod_equalise_tables_device(_ptr(pic), _ptr(val), EQ_W, EQ_H, EQ_PLANES, C.byref(o), _ptr(work), need, d, st), "mdemod_equalise_tables_device")
            return [work]
        out = ctx.guarded(tuple(pic.shape), torch.uint8)
        if stage == "apply":
            _check(lib.mdemod_equalise_apply_device(_ptr(pic), _ptr(val), EQ_W, EQ_H, EQ_PLANES, C.byref(o), _ptr(dev["work"]), _ptr(out), d, st),
                    "mdemod_equalise_apply_device")
            return [out]
        work = ctx.guarded((need,), torch.uint8)
        _check(lib.mdemod_equalise_device(_ptr(pic), _ptr(val), EQ_W, EQ_H, EQ_PLANES, C.byref(o), _ptr(work), need, _ptr(out), d, st), "mdemod_equalise_device")
        return [out, work]
    return call


def _equalise_rows() -> list:
    L = "equalise"
    return [
        Row("mdemod_equalise_tables_device", L, "async", _eq_inputs, lambda inp: [_eq_work(inp)], _call_eq("tables")),
        Row("mdemod_equalise_apply_device", L, "async", _eq_apply_inputs, lambda inp: [_eq_out(inp)], _call_eq("apply")),
        Row("mdemod_equalise_device", L, "async", _eq_inputs, lambda inp: [_eq_out(inp), _eq_work(inp)], _call_eq("both")),
    ]


# =============================================================================================================================== sun
def _sun_inputs(which: str) -> dict:
    import sun_util as SU
    pics = SU.pictures(1, seed={"real": 11, "poison": 12}[which])
    return {"im0": pics[0], "im1": pics[1], "im2": pics[2], "gain": _i32(SU.gain_table("synthetic", 1))}


def _sun_expected(inp):
    from meteor_demod_amd import sun
    outs, sat = sun.model_apply([inp["im0"], inp["im1"], inp["im2"]], inp["gain"].view(np.uint32), (0, 1, 2))
    return [outs[0], outs[1], outs[2], np.array(sat, dtype=np.int64)]


def _call_sun(dev, ctx):
    import torch
    from meteor_demod_amd import sun
    ims = [dev["im0"], dev["im1"], dev["im2"]]
    outs, work = sun.apply_tensors(ims, dev["gain"], (0, 1, 2), out=[ctx.guarded(tuple(t.shape), torch.uint8) for t in ims])
    return [outs[0], outs[1], outs[2], lambda: work.to(torch.int64).sum(dim=0).cpu().numpy()]


def _sun_rows() -> list:
    return [Row("mdemod_sun_apply_device", "sun", "async", _sun_inputs, _sun_expected, _call_sun)]


# ====================================================================================================================== jpeg and png
ENC_W, ENC_H, ENC_PLANES, JPEG_Q, JPEG_RST, PNG_SEGMENT = 64, 64, 3, 90, 32, 0


def _file_same(got, want):
    """(the output buffer, the result words or the byte count) against (the file's bytes): the count, then the bytes."""
    n = int(np.asarray(got[1]).reshape(-1)[0])
    assert n == len(want[0]), (n, len(want[0]))
    assert np.array_equal(np.asarray(got[0]).reshape(-1)[:n], want[0]), "the file's bytes differ"


def _bytes(b: bytes) -> list:
    return [np.frombuffer(b, dtype=np.uint8)]


def _jpeg_inputs(which: str) -> dict:
    import jpeg_cases as JC
    return {"picture": JC.picture(ENC_W, ENC_H, ENC_PLANES, seed={"real": 0, "poison": 1}[which])}


def _jpeg_coef_inputs(which: str) -> dict:
    from meteor_demod_amd import jpeg
    return {"coef": jpeg.model_coefficients(_jpeg_inputs(which)["picture"], JPEG_Q)}


def _png_inputs(which: str) -> dict:
    import png_cases as PC
    seed = {"real": 0, "poison": 1}[which]
    return {"picture": PC.picture(ENC_W, ENC_H, ENC_PLANES, seed=seed), "valid": PC.mask(ENC_W, ENC_H, seed=seed)}


def _png_bytes_inputs(which: str) -> dict:
    from meteor_demod_amd import png
    d = _png_inputs(which)
    return {"data": np.ascontiguousarray(png.model_filter(d["picture"], d["valid"])).reshape(-1)}


def _encoder_call(layer: str, stage: str, with_result: bool):
    """The device entry of ``layer`` ("jpeg" / "png") and ``stage`` ("encode" / "second") with the wrappers' own scratch memory; with
    ``with_result`` the layer's result entry behind it, which waits for the stream and hands the byte count back."""
    def call(dev, ctx):
        from meteor_demod_amd import _encode, jpeg, png
        if layer == "jpeg":
            lib = jpeg.lib()
            if stage == "encode":
                s = _encode.Scratch(dev["picture"], jpeg.bound(ENC_W, ENC_H, ENC_PLANES, JPEG_RST), jpeg.workspace(ENC_W, ENC_H, ENC_PLANES, JPEG_RST))
                _check(lib.mdemod_jpeg_encode_device(_ptr(dev["picture"]), ENC_W, ENC_H, ENC_PLANES, JPEG_Q, JPEG_RST, *s.tail), "mdemod_jpeg_encode_device")
            else:
                n_mcus = int(dev["coef"].shape[0]) // ENC_PLANES
                s = _encode.Scratch(dev["coef"], int(lib.mdemod_jpeg_entropy_bound(n_mcus, ENC_PLANES, JPEG_RST)), int(lib.mdemod_jpeg_entropy_workspace(n_mcus, JPEG_RST)))
                _check(lib.mdemod_jpeg_entropy_device(_ptr(dev["coef"]), n_mcus, ENC_PLANES, JPEG_RST, *s.tail), "mdemod_jpeg_entropy_device")
            result, name = lib.mdemod_jpeg_result, "mdemod_jpeg_result"
        else:
            lib = png.lib()
            if stage == "encode":
                s = _encode.Scratch(dev["picture"], png.bound(ENC_W, ENC_H, ENC_PLANES, True, PNG_SEGMENT), png.workspace(ENC_W, ENC_H, ENC_PLANES, True, PNG_SEGMENT))
                _check(lib.mdemod_png_encode_device(_ptr(dev["picture"]), _ptr(dev["valid"]), ENC_W, ENC_H, ENC_PLANES, png.FILTER_ADAPT, PNG_SEGMENT, *s.tail),
                          "mdemod_png_encode_device")
            else:
                n = int(dev["data"].shape[0])
                s = _encode.Scratch(dev["data"], png.deflate_bound(n, PNG_SEGMENT), int(lib.mdemod_png_deflate_workspace(n, PNG_SEGMENT)))
                _check(lib.mdemod_png_deflate_device(_ptr(dev["data"]), n, PNG_SEGMENT, *s.tail), "mdemod_png_deflate_device")
            result, name = lib.mdemod_png_result, "mdemod_png_result"
        ctx.state["scratch"] = s
        if not with_result:
            return [s.out, s.result]
        n = C.c_uint64()
        _check(result(_ptr(s.result), C.byref(n), s.d, s.stream), name)
        return [s.out, np.array([n.value], dtype=np.int64)]
    return call


def _encoder_rows() -> list:
    from meteor_demod_amd import jpeg, png
    jpeg_file = lambda inp: _bytes(jpeg.model_encode(inp["picture"], JPEG_Q, JPEG_RST))
    png_file = lambda inp: _bytes(png.model_encode(inp["picture"], inp["valid"], png.FILTER_ADAPT, PNG_SEGMENT))
    return [
        Row("mdemod_jpeg_encode_device", "jpeg", "async", _jpeg_inputs, jpeg_file, _encoder_call("jpeg", "encode", False), _file_same),
        Row("mdemod_jpeg_entropy_device", "jpeg", "async", _jpeg_coef_inputs, lambda inp: _bytes(jpeg.model_entropy(inp["coef"], ENC_PLANES, JPEG_RST)),
            _encoder_call("jpeg", "second", False), _file_same),
        Row("mdemod_jpeg_result", "jpeg", "sync", _jpeg_inputs, jpeg_file, _encoder_call("jpeg", "encode", True), _file_same),
        Row("mdemod_png_encode_device", "png", "async", _png_inputs, png_file, _encoder_call("png", "encode", False), _file_same),
        Row("mdemod_png_deflate_device", "png", "async", _png_bytes_inputs, lambda inp: _bytes(png.model_deflate(inp["data"], PNG_SEGMENT)),
            _encoder_call("png", "second", False), _file_same),
        Row("mdemod_png_result", "png", "sync", _png_inputs, png_file, _encoder_call("png", "encode", True), _file_same),
    ]


# ========================================================================================================================= the table
@_cached
def rows() -> tuple:
    out = (_demod_rows() + _internal_rows() + _fe_rows() + _survey_rows() + _frames_rows() + _il_rows() + _rs_rows() + _image_rows() + _picture_rows() + _map_rows() + _mosaic_rows()
           + _polar_rows() + _overlay_rows() + _equalise_rows() + _sun_rows() + _encoder_rows())
    return tuple(out)


@_cached
def extra_rows() -> tuple:
    """Second cases of functions that have their row in the table: run by the same tests, not counted by the completeness test."""
    return tuple(_il_extra_rows())


def all_rows() -> tuple:
    return rows() + extra_rows()


def by_name() -> dict:
    return {r.key: r for r in all_rows()}


@functools.lru_cache(maxsize=None)
def case(function: str, which: str) -> dict:
    """A row's inputs, made once."""
    d = by_name()[function].inputs(which)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def want(function: str, which: str) -> tuple:
    """A row's expected outputs for its real or its poison input, computed once."""
    return tuple(by_name()[function].expected(case(function, which)))


# The exported entries outside include/ that the table covers as well: the setters of the recording stitcher, which the Python
# wrapper offers (Demodulator.rotate_carrier, set_*_seeds).  The rest of that header is reached through mdemod_demodulate_recording.
INTERNAL_HEADER = "meteor_demod_amd/csrc/mdemod_internal_api.h"
INTERNAL = ("mdemod_rotate_carrier", "mdemod_set_carrier_seeds", "mdemod_set_gain_seeds", "mdemod_set_clock_seeds")


def _stream_declarations(path) -> list:
    import re
    text = re.sub(r"/\*.*?\*/", " ", path.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return [m.group(1) for m in re.finditer(r"\b(mdemod_\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bhip_stream\b", m.group(2))]


def declared() -> dict:
    """{function: header, as a path from the repository's root} of every declaration in include/*.h whose parameter list holds
    ``hip_stream``, and of the entries ``INTERNAL`` of csrc/mdemod_internal_api.h."""
    from conftest import ROOT
    out = {}
    for path in sorted((ROOT / "include").glob("*.h")):
        for name in _stream_declarations(path):
            assert name not in out, f"{name} is declared in {out[name]} and in {path.name}"
            out[name] = f"include/{path.name}"
    internal = ROOT / INTERNAL_HEADER
    if internal.exists():
        found = _stream_declarations(internal)
        for name in INTERNAL:
            assert name in found and name not in out, f"{name}: not declared with a hip_stream parameter in {INTERNAL_HEADER} alone"
            out[name] = INTERNAL_HEADER
    return out
