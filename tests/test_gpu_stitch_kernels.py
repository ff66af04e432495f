"""The recording stitcher's kernels (csrc/recording.hip), each against its plain model (tests/stitch_ref.py): the three seam
matches and the assembly copy exactly, the AGC power with a derived bound, the carrier and clock estimators against float64
with a tolerance the model measures on itself.  The whole-recording tests (test_gpu_recording.py) hold the stitcher to
statistical bars; a wrong tie rule, a group border of the copy or a decimation factor nobody runs would sit under those.

The kernels are reached through mdemod_selftest_seam_match / _assemble / _window_power, which run the stitcher's own launch code
(run_match, run_assemble, run_window_power), and through the estimator entries the stitcher itself calls."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import stitch_cases as SC
import stitch_ref as R
from meteor_demod_amd import DemodConfig, _capi, synth
from meteor_demod_amd import recording as REC

pytestmark = pytest.mark.gpu

MATCH = (R.match_tails, R.match_rails, R.match_heads)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# ---- seam matches ------------------------------------------------------------------------------------------------------------

def _model_of(mode, K, p):
    if mode == 0:
        return R.match_tails(p["a"], p["b"], K, b_rot=p["b_rot"], force_weak=p["force_weak"])
    return MATCH[mode](p["a"], p["b"], K, force_weak=p["force_weak"])


def _assert_batch_covers_every_class(mode, K, pairs, model):
    """On the CPU, with the model alone: the batch holds what it is meant to hold."""
    tail = K + 2 if mode == 1 else K + 1
    live = [(p, m) for p, m in zip(pairs, model) if not m["weak"]]
    if mode == 1:
        for r in range(4):
            for d in (-1, 0, 1):
                assert any(p.get("want") == (0, r, d) and m["rot"] == r and m["pairing"][r] == (d, d) for p, m in live), (r, d)
    else:
        assert {(m["shift"], m["rot"]) for _, m in live} == set(SC.SHIFT_ROT)
        assert all((m["shift"], m["rot"]) == p["want"][:2] for p, m in live if "want" in p)
    rule = lambda m: 4 * m["best"] ** 2 < m["ea"] * m["eb"]
    assert any(m["weak"] and m["best"] <= 0 for m in model)
    assert any(m["weak"] and m["best"] > 0 and rule(m) and not p["force_weak"] for p, m in zip(pairs, model))
    assert sum(1 for p, m in zip(pairs, model) if p["force_weak"] and m["best"] > 0 and not rule(m)) >= 12      # forced, would have matched
    if mode == 1:
        assert any(m["tots"].count(m["best"]) >= 2 and m["best"] > 0 for m in model)                          # two rotations tie
        assert any(m["tots"].count(m["best"]) >= 2 and m["tots"][0] != m["best"] for m in model)              # ... and not with rotation 0
    else:
        top = lambda m: [max(re, im, -re, -im) for _, re, im in m["scores"]]
        assert any(top(m).count(m["best"]) >= 2 and m["best"] > 0 for m in model)                             # two shifts tie
        assert any(top(m)[0] < m["best"] and top(m)[1] == top(m)[2] == m["best"] for m in model)              # +1 and -1 tie, 0 is out
        win = lambda m: next([re, im, -re, -im] for s, re, im in m["scores"] if s == m["raw_shift"])
        assert any(win(m).count(m["best"]) >= 2 and m["best"] > 0 for m in model)                             # two rotations tie
    assert any(m["best"] > 0 and 4 * m["best"] ** 2 == m["ea"] * m["eb"] and not m["weak"] for m in model)    # on the boundary
    assert any(0 < m["ea"] * m["eb"] - 4 * m["best"] ** 2 <= m["eb"] and m["weak"] for m in model)            # one count of Ea below it
    cnts = [(len(p["a"]), len(p["b"])) for p in pairs]
    assert any(a >= K + 8 and b >= K + 8 and a != b for a, b in cnts)
    for c in (tail, K, 1, 0):
        assert any(a == c for a, _ in cnts) and any(b == c for _, b in cnts), c
    assert any(len(p["a"]) > K and np.abs(p["a"]).min() == 127 and np.abs(p["b"]).min() == 127 and not m["weak"] for p, m in live)
    if mode == 0:
        assert {p["b_rot"] for p, _ in live} == {0, 1, 2, 3}
    kinds = [p["kind"] for p in pairs]
    assert all(x != y for x, y in zip(kinds[:100], kinds[1:101]))                                             # neighbouring blocks differ in kind
    assert 190 <= len(pairs) <= 260


@pytest.mark.parametrize("K", [32, 100, 192, 257])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=SC.MODES)
def test_seam_matches_equal_the_model(mode, K, gpu_device):
    """match_kernel, match_rails_kernel, match_heads_kernel: shift, rotation and weak flag of every pair of a batch of about 200
    equal the integer model's.  The batch holds all 12 (shift, rotation) answers, the three reasons for a weak pair, exact ties
    between shifts and between rotations, the weak boundary itself and one count below it, tails longer than, as long as and
    shorter than the compared stretch down to 1 and 0 symbols, full-scale symbols, B stored turned (tails) and forced pairs."""
    pairs = SC.seam_batch(mode, K)
    model = [_model_of(mode, K, p) for p in pairs]
    _assert_batch_covers_every_class(mode, K, pairs, model)
    abuf, a_off, a_cnt = SC.pack(pairs, "a")
    bbuf, b_off, b_cnt = SC.pack(pairs, "b")
    shift, rot, weak = REC.selftest_seam_match(mode, _dev(abuf), _dev(bbuf), a_off, a_cnt, b_off, b_cnt,
                                               [p["b_rot"] for p in pairs], [p["force_weak"] for p in pairs], K)
    want = np.array([(m["shift"], m["rot"], m["weak"]) for m in model])
    got = np.stack((shift, rot, weak), axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, [(int(j), pairs[j]["kind"], got[j].tolist(), want[j].tolist()) for j in bad[:10]]


def test_seam_match_entry_refuses_what_it_cannot_run(gpu_device):
    import torch
    buf = torch.zeros((64, 2), dtype=torch.int8, device="cuda")
    one = dict(a_off=[0], a_cnt=[40], b_off=[0], b_cnt=[40], force_weak=[0])

    def refused(word, mode, a, b, K, b_rot=(0,), **kw):
        args = dict(one, **kw)
        with pytest.raises(_capi.MdemodError) as e:
            REC.selftest_seam_match(mode, a, b, args["a_off"], args["a_cnt"], args["b_off"], args["b_cnt"], list(b_rot), args["force_weak"], K)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail

    for mode in range(3):
        refused("K", mode, buf, buf, 0)
        refused("K", mode, buf, buf, -5)
        refused("a_dev", mode, None, buf, 32)
        refused("b_dev", mode, buf, None, 32)
        refused("a_cnt", mode, buf, buf, 32, a_cnt=[65])                       # reaches past the buffer
        refused("b_off", mode, buf, buf, 32, b_off=[30])
    refused("b_rot", 1, buf, buf, 32, b_rot=(1,))
    refused("b_rot", 2, buf, buf, 32, b_rot=(3,))
    refused("mode", 3, buf, buf, 32)
    for mode in range(3):                                                       # no pairs: nothing to do, whatever the buffers
        sh, ro, we = REC.selftest_seam_match(mode, None, None, [], [], [], [], [], [], 32)
        assert len(sh) == len(ro) == len(we) == 0
    sh, ro, we = REC.selftest_seam_match(0, buf, buf, [0], [40], [0], [40], [2], [0], 32)      # b_rot is mode 0's to take
    assert (int(sh[0]), int(ro[0]), int(we[0])) == (0, 0, 1)


# ---- assembly ----------------------------------------------------------------------------------------------------------------

CANARY = 0x5A


@pytest.mark.parametrize("T", [1, 3, 70, 2049])
def test_assembly_copy_equals_the_model_byte_for_byte(T, gpu_device):
    """assemble_kernel through the stitcher's launch (slices = min(64, max(1, 4096 / T))): every byte of the output equals the
    model's - the tiles' symbols turned and in place, the canaries in front, behind and in the one gap untouched - and the source
    is unchanged.  keep runs through the borders of the 16-byte groups (0, 1, 7, 8, 9, 15, 16, 17) and of a slice's loop
    (8 * 256 * slices - 1, that, + 9, three times that + 5); rotations, head symbols and their rotations cycle independently,
    one head sits on a tile with nothing to keep; offsets of both parities on either side; the source holds -128 and +-127."""
    import torch
    slices = min(64, max(1, 4096 // T))
    P = 8 * 256 * slices
    rng = np.random.default_rng(T)
    keeps = [0, 1, 7, 8, 9, 15, 16, 17, P - 1, P, P + 9, 3 * P + 5]
    n_src = 3 * P + 5 + 4096
    src = rng.integers(-128, 128, size=(n_src, 2)).astype(np.int8)
    src[::97] = (-128, 127)
    src[5::101] = (-127, -128)
    if T == 1:
        runs = [[k] for k in (3 * P + 5, P - 1, P, P + 9, 9, 0)]
    elif T == 3:
        runs = [[P + 9, 0, 3 * P + 5], [17, P - 1, P]]
    else:
        runs = [[keeps[(t + T) % len(keeps)] for t in range(T)]]
    d_src = _dev(src)
    seen_rot, seen_head, parity = set(), set(), set()
    for run, keep in enumerate(runs):
        keep = np.array(keep, dtype=np.uint32)
        t = np.arange(T) + run
        rot = (t % 4).astype(np.int32)
        has_head = (t % 3 == 1) | (keep == 0)
        head_off = np.where(has_head, rng.integers(0, n_src, size=T), -1).astype(np.int64)
        head_rot = ((t // 3) % 4).astype(np.int32)
        src_off = np.array([rng.integers(0, n_src - int(k) + 1) for k in keep], dtype=np.uint64)
        src_off[: T // 2] |= 1
        src_off = np.minimum(src_off, n_src - keep.astype(np.uint64))
        room = keep.astype(np.int64) + has_head
        dst = 37 + np.concatenate(([0], np.cumsum(room)[:-1]))
        if T >= 3:
            dst[T // 2:] += 3                                                   # one gap: the tiles abut everywhere else
        n_out = int(dst[-1] + room[-1]) + 41
        out0 = np.full((n_out, 2), CANARY, dtype=np.int8)
        want = R.assemble(out0.copy(), src, src_off, keep, rot, head_off, head_rot, dst)
        assert (want[:37] == CANARY).all() and (want[-41:] == CANARY).all()
        d_out = _dev(out0)
        REC.selftest_assemble(d_src, d_out, src_off, keep, rot, head_off, head_rot, dst)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (T, keep[:12].tolist(), bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        seen_rot |= set(rot[keep > 0].tolist())
        seen_head |= set(head_rot[has_head].tolist())
        parity |= {(int(s) & 1, int(d) & 1) for s, d, k in zip(src_off, dst + has_head, keep) if k >= 8}
    assert np.array_equal(d_src.cpu().numpy(), src)
    if T > 3:
        assert seen_rot == {0, 1, 2, 3} and seen_head == {0, 1, 2, 3} and parity == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert set(keeps) <= set(runs[0]) and any(k == 0 and h for k, h in zip(keep, has_head))
    with pytest.raises(_capi.MdemodError) as e:                                  # a table that reaches past the output is refused, not run
        REC.selftest_assemble(d_src, d_out, [0], [16], [0], [-1], [0], [n_out - 15])
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "dst" in e.value.detail


# ---- window power ------------------------------------------------------------------------------------------------------------

def _power_bound(x, n):
    """See test_window_power_within_its_derived_bound."""
    u = 2.0 ** -24
    gamma = lambda k: k * u / (1 - k * u)
    depth = (n + 255) // 256 - 1 + 8                      # additions on the longest path: serial per thread, then the tree of 256
    e2 = sum((gamma(depth + 1) * float(np.mean(np.abs(x[:, c])))) ** 2 for c in (0, 1))
    z = x[:, 0] + 1j * x[:, 1]
    p = float(np.mean(np.abs(z - z.mean()) ** 2))
    return gamma(depth + 5) * (p + e2) + e2


@pytest.mark.parametrize("bps", [8, 16, 32])
def test_window_power_within_its_derived_bound(bps, gpu_device):
    """window_power_kernel through the stitcher's launch against the float64 mean of |z - mean|^2, for n = 0, 1, 255, 256, 257 and
    4099 samples from odd and even starts, and one window whose DC level is a thousand times its spread (s16 and f32; u8 has no
    room for one).

    The bound follows the kernel's order of summation.  Samples are exact in float32.  Thread t adds its m = ceil(n / 256) terms
    serially, then a tree of 8 levels adds the 256 partial sums: no term passes through more than D = m - 1 + 8 additions, so
    a computed sum is sum x_k (1 + d_k) with |d_k| <= g(D), g(k) = k u / (1 - k u), u = 2^-24.  The mean (one more rounding for the
    division) is off by at most e_c = g(D + 1) * mean|x_c| per component c.  The second pass computes |z_k - m|^2 with four
    roundings per term (two differences squared: 2u + u each, one addition: in all below g(4)), sums them (g(D)) and divides (u):
    P^ = (1 / n) sum |z_k - m^|^2 (1 + t_k), |t_k| <= g(D + 5).  Because sum (z_k - mean) = 0, (1 / n) sum |z_k - m^|^2 = P + |e|^2
    exactly: the error of the mean adds its own square.  So |P^ - P| <= g(D + 5) (P + |e|^2) + |e|^2 with |e|^2 = e_re^2 + e_im^2.
    No fused multiply-add shortens this: the library is built with -ffp-contract=off."""
    rng = np.random.default_rng(bps)
    n_iq = 20000
    if bps == 8:
        iq = rng.integers(0, 256, size=(n_iq, 2)).astype(np.uint8)
    elif bps == 16:
        iq = rng.integers(-32768, 32768, size=(n_iq, 2)).astype(np.int16)
        iq[9000:13200] = rng.integers(-10, 11, size=(4200, 2)) + (20000, -20000)
    else:
        iq = rng.normal(0, 0.3, size=(n_iq, 2)).astype(np.float32)
        iq[9000:13200] = (rng.uniform(-0.5, 0.5, size=(4200, 2)) + (1000.0, -1000.0)).astype(np.float32)
    starts, lens = [], []
    for n in (0, 1, 255, 256, 257, 4099):
        for s in (1234, 4321):
            starts.append(s), lens.append(n)
    if bps != 8:
        starts += [9001, 9050]
        lens += [4099, 4100]
    starts.append(n_iq - 257), lens.append(257)                                   # up to the very end
    got = REC.selftest_window_power(DemodConfig(samplerate=230000, bps=bps), _dev(iq), starts, lens)
    x = R.to_float(iq)
    worst = 0.0
    for s, n, g in zip(starts, lens, got):
        want = R.window_power(iq, s, n)
        if n == 0:
            assert g == 0.0
            continue
        bound = _power_bound(x[s:s + n], n)
        print(f"window_power bps {bps} start {s} n {n}: model {want:.9g} kernel {float(g):.9g} deviation {abs(float(g) - want):.3g} bound {bound:.3g}")
        assert abs(float(g) - want) <= bound, (s, n, float(g), want, bound)
        worst = max(worst, abs(float(g) - want) / bound)
    print(f"window_power bps {bps}: largest deviation / bound {worst:.3f}")
    with pytest.raises(_capi.MdemodError) as e:
        REC.selftest_window_power(DemodConfig(samplerate=230000, bps=bps), _dev(iq), [n_iq - 10], [11])
    assert e.value.code == _capi.MDEMOD_ERR_PARAM and "lens" in e.value.detail


# ---- carrier and clock estimators --------------------------------------------------------------------------------------------

MARGIN = 1.01           # the model's largest in-band magnitude over its second largest non-neighbour: the peak bin is not a toss-up
FACTOR = 16.0           # float32 butterflies and twiddles of the kernel's FFT: about log2(NF) roundings per point


@functools.lru_cache(maxsize=None)
def _estimator_models():
    """Every case's inputs and float64 model, once; and the tolerance: the largest change of a line's fractional position (bins)
    and of a quality (relative) when the model rounds its windowed, decimated sequence to float32 before the FFT and the three
    magnitudes to float32 before Grandke, over all cases, times FACTOR."""
    cases, dev_pos, dev_q = {}, 0.0, 0.0
    for name, (fs, sr, oq, bps, window, geo, *_r) in SC.CARRIER_CASES.items():
        nwin, decim, l2, kmax, pre = R.carrier_geometry(fs, sr, window)
        assert (decim, pre) == geo, name
        iq, chirp = SC.carrier_inputs(synth, name)
        starts = SC.estimator_windows(nwin)
        m = R.carrier_estimate(iq, fs, sr, oq, starts, window, chirp=chirp)
        mr = R.carrier_estimate(iq, fs, sr, oq, starts, window, chirp=chirp, round_seq=True, round_mags=True)
        cases[("carrier", name)] = dict(iq=iq, starts=starts, chirp=chirp, model=m, nwin=nwin)
        for a, b in zip(m[:2], mr[:2]):
            assert a["k"] == b["k"]
            dev_pos, dev_q = max(dev_pos, abs(a["delta"] - b["delta"])), max(dev_q, abs(b["quality"] / a["quality"] - 1))
    for name, (fs, sr, oq, bps, window, decim, *_r) in SC.CLOCK_CASES.items():
        assert R.clock_geometry(fs, sr, oq, window)[:2] == (window, decim), name
        st, iq, carrier, chirp = SC.clock_inputs(synth, name, window)
        starts = SC.estimator_windows(window)
        interp = DemodConfig(samplerate=fs).interp_factor
        m = R.clock_estimate(iq, fs, sr, oq, interp, starts, window, carrier=carrier, chirp=chirp)
        mr = R.clock_estimate(iq, fs, sr, oq, interp, starts, window, carrier=carrier, chirp=chirp, round_seq=True, round_mags=True)
        cases[("clock", name)] = dict(iq=iq, starts=starts, carrier=carrier, chirp=chirp, model=m, nwin=window, interp=interp)
        for a, b in zip(m[:2], mr[:2]):
            assert a["k"] == b["k"]
            dev_pos = max([dev_pos] + [abs(x - y) for x, y in zip(a["delta"], b["delta"])])
            dev_q = max(dev_q, abs(b["quality"] / a["quality"] - 1))
    assert 0 < dev_pos < 1e-6 and 0 < dev_q < 1e-6            # (a float32 rounding of three magnitudes: a few 1e-8)
    return cases, dev_pos, dev_q, FACTOR * dev_pos, FACTOR * dev_q


def _between(x, lo, hi):
    return min(lo, hi) <= x <= max(lo, hi)


def _f32(x):
    return np.float32(x)


@pytest.mark.parametrize("name", list(SC.CARRIER_CASES))
def test_carrier_estimator_against_the_float64_model(name, gpu_device):
    """carrier_line_kernel at every decimation and pre-averaging factor it has, on u8, s16 and f32, with and without the
    de-chirp, for a window inside the recording, one half over its end and one wholly past it (a constant: all zero after the
    mean removal, the tie rule puts the peak on the lowest bin searched, quality 0).  Inputs are synthetic streams at 12 dB whose
    model peak stands at least 1 % above every bin that is not its neighbour (checked here).  The peak bin is the model's; the
    line's fractional position and the quality are the model's to within 16 times what float32 roundings of the FFT's input and of
    the three magnitudes move them by in the model itself.

    The kernel reports float32((k + delta) * Hz per bin * rad per Hz), three float32 roundings on the way: a position is only
    known up to the set of positions that give the same word.  The position is held to the tolerance where it can be told: the
    kernel's word must lie between the words the model's k and delta -+ tolerance give through the same three roundings (each
    is monotone).  Nothing is added to the tolerance."""
    cases, dev_pos, dev_q, tol_pos, tol_q = _estimator_models()
    c = cases[("carrier", name)]
    fs, sr, oq, bps, window, *_r = SC.CARRIER_CASES[name]
    cfg = DemodConfig(samplerate=fs, symrate=sr, oqpsk=oq, bps=bps)
    freq, qual, used = REC.estimate_carrier_native(cfg, _dev(c["iq"]), c["starts"], window, chirp=c["chirp"])
    freq, qual = freq.cpu().numpy(), qual.cpu().numpy()
    assert used == c["nwin"]
    hz, rad = _f32(fs / c["nwin"] / 4.0), _f32(2 * math.pi / (sr * (2 if oq else 1)))
    word = lambda k, d: _f32(_f32(_f32(_f32(k) + _f32(d)) * hz) * rad)
    for w, m in enumerate(c["model"]):
        assert m["margin"] >= MARGIN, (name, w, m["margin"])
        pos = float(freq[w]) / (float(hz) * float(rad))
        kdev, qdev = abs(pos - m["k"] - m["delta"]), (abs(float(qual[w]) / m["quality"] - 1) if m["quality"] else abs(float(qual[w])))
        print(f"carrier {name} window {w}: bin {m['k']} delta {m['delta']:+.7f} quality {m['quality']:.4f}; kernel word -> {pos:.7f} bins "
              f"(off by {kdev:.2e}, tolerance {tol_pos:.2e} = {FACTOR:g} x {dev_pos:.2e}), quality {float(qual[w]):.4f} (off by {qdev:.2e}, tolerance {tol_q:.2e} = {FACTOR:g} x {dev_q:.2e})")
        if w == 2:
            assert m["k"] == -m["kmax"] + 1 and m["delta"] == 0 and m["quality"] == 0
            assert float(freq[w]) == float(word(m["k"], 0.0)) and float(qual[w]) == 0.0
            continue
        assert round(pos - m["delta"]) == m["k"], (name, w, pos, m["k"], m["delta"])
        assert _between(freq[w], word(m["k"], m["delta"] - tol_pos), word(m["k"], m["delta"] + tol_pos)), (name, w, pos, m["k"] + m["delta"], tol_pos)
        assert _between(qual[w], _f32(m["quality"] * (1 - tol_q)), _f32(m["quality"] * (1 + tol_q))), (name, w, float(qual[w]), m["quality"], tol_q)


@pytest.mark.parametrize("name", list(SC.CLOCK_CASES))
def test_clock_estimator_against_the_float64_model(name, gpu_device):
    """clock_line_kernel without shuffles (decim 1), with them (16) and with one wave per group (64, u8 and f32), QPSK and OQPSK,
    the latter with its carrier and a chirp taken out; windows, inputs, margin and tolerance as for the carrier estimator.  The
    recording ends on a zero sample, so the window past the end is zero throughout (there is no mean removal here).

    The kernel reports float32((f_nom + pos / nwin) * 2 pi / interp) with pos = float32(k + delta) (OQPSK: half the distance
    of two such): one step of the word is worth 1e-4 bin of a 4096-sample window and 6e-3 bin of a 2^18 one.  As for the carrier,
    the kernel's word must lie between the words that the model's lines, each moved by the tolerance, give through the same
    roundings.

    (This test found the per-step rotation of the kernel's phasors made from a float32 phase: quality 8.5e-7 off where
    7.2e-7 is allowed.  With the step taken from the double-precision phase the largest deviation is 1.6e-7.)"""
    cases, dev_pos, dev_q, tol_pos, tol_q = _estimator_models()
    c = cases[("clock", name)]
    fs, sr, oq, bps, window, *_r = SC.CLOCK_CASES[name]
    cfg = DemodConfig(samplerate=fs, symrate=sr, oqpsk=oq, bps=bps)
    tf, qual = REC.estimate_clock_native(cfg, _dev(c["iq"]), c["starts"], window, carrier=c["carrier"], chirp=c["chirp"])
    tf, qual = tf.cpu().numpy(), qual.cpu().numpy()
    f_nom, scale, nwin = sr / fs, 2 * math.pi / c["interp"], c["nwin"]
    line = lambda k, d: float(_f32(_f32(k) + _f32(d)))

    def word(k, d, sign):
        p = [line(kk, dd + sg * sign * tol_pos) for kk, dd, sg in zip(k, d, (1, -1))]
        return _f32((f_nom + (0.5 * (p[0] - p[1]) if oq else p[0]) / nwin) * scale)

    for w, m in enumerate(c["model"]):
        assert m["margin"] >= MARGIN, (name, w, m["margin"])
        pos = (float(tf[w]) / scale - f_nom) * nwin
        cell = float(np.spacing(tf[w])) / scale * nwin
        qdev = abs(float(qual[w]) / m["quality"] - 1) if m["quality"] else abs(float(qual[w]))
        print(f"clock {name} window {w}: bins {m['k']} position {m['pos']:+.7f} quality {m['quality']:.4f}; kernel word -> {pos:+.7f} bins "
              f"(off by {abs(pos - m['pos']):.2e}; one step of the word is {cell:.2e} bins; tolerance {tol_pos:.2e} = {FACTOR:g} x {dev_pos:.2e}), "
              f"quality {float(qual[w]):.4f} (off by {qdev:.2e}, tolerance {tol_q:.2e} = {FACTOR:g} x {dev_q:.2e})")
        if w == 2:
            assert all(k == -m["kmax"] + 1 for k in m["k"]) and m["quality"] == 0
            assert float(tf[w]) == float(_f32((f_nom + m["pos"] / nwin) * scale)) and float(qual[w]) == 0.0
            continue
        # the peak bins, as far as the word shows them: the line's own (QPSK), the distance of the two (OQPSK)
        if oq:
            assert round(2 * pos - (m["delta"][0] - m["delta"][1])) == m["k"][0] - m["k"][1], (name, w, pos, m["k"], m["delta"])
        else:
            assert round(pos - m["delta"][0]) == m["k"][0], (name, w, pos, m["k"], m["delta"])
        assert _between(tf[w], word(m["k"], m["delta"], -1), word(m["k"], m["delta"], +1)), (name, w, pos, m["pos"], tol_pos, cell)
        assert _between(qual[w], _f32(m["quality"] * (1 - tol_q)), _f32(m["quality"] * (1 + tol_q))), (name, w, float(qual[w]), m["quality"], tol_q)
