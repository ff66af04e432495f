"""The plain models of the stitcher's kernels (tests/stitch_ref.py) against answers that were planted: what the GPU tests
compare the kernels with has to be right by itself.  No GPU."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import stitch_cases as SC
import stitch_ref as R
from meteor_demod_amd import DemodConfig, _capi, synth

MATCH = (R.match_tails, R.match_rails, R.match_heads)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=SC.MODES)
@pytest.mark.parametrize("K", [32, 192])
def test_planted_shift_and_rotation_come_back(mode, K):
    """A copy of A turned by r and displaced by s, with +-10 of noise on symbols of 40..100, answers exactly (s, r): all 12 pairs
    (rails: every rotation with the rails paired at -1, 0 and +1, and at different shifts)."""
    rng = np.random.default_rng(5 + mode)
    for s, r in SC.SHIFT_ROT:
        for noise in (0, 10):
            if mode == 1:
                for dq in (-1, 0, 1):
                    p = SC.planted(mode, rng, K, 0, r, K + 8, K + 11, noise=noise, d_i=s, d_q=dq)
                    m = R.match_rails(p["a"], p["b"], K)
                    assert (m["rot"], m["weak"], m["pairing"][r]) == (r, 0, (s, dq)), (s, r, dq, m)
            else:
                p = SC.planted(mode, rng, K, s, r, K + 8, K + 11, noise=noise)
                m = MATCH[mode](p["a"], p["b"], K)
                assert (m["shift"], m["rot"], m["weak"]) == (s, r, 0), (s, r, m)
                assert 4 * m["best"] ** 2 > 3 * m["ea"] * m["eb"]                    # nearly a perfect match, not merely above the rule
    # b_rot (tails): B stored k quarter turns back is the same pair
    for k in range(4):
        p = SC.planted(0, rng, K, 1, 3, K + 8, K + 8, b_rot=k)
        m = R.match_tails(p["a"], p["b"], K, b_rot=k)
        assert (m["shift"], m["rot"], m["weak"]) == (1, 3, 0)
        if k:
            assert R.match_tails(p["a"], p["b"], K)["rot"] == (3 + k) % 4             # not applied: the answer turns with it


@pytest.mark.parametrize("mode", [0, 1, 2], ids=SC.MODES)
def test_unrelated_and_empty_tails_are_weak_and_forcing_works(mode):
    K = 100
    rng = np.random.default_rng(11)
    f = MATCH[mode]
    for _ in range(20):
        m = f(SC._base(rng, K + 8), SC._base(rng, K + 8), K)
        assert m["weak"] == 1 and (m["shift"], m["rot"]) == (0, 0) and m["best"] > 0     # weak by the energy rule
    z = np.zeros((K + 8, 2), dtype=np.int64)
    for a, b in ((z, z), (z, SC._base(rng, K + 8)), (SC._base(rng, K + 8), z), (z[:0], z[:0])):
        m = f(a, b, K)
        assert m["weak"] == 1 and m["best"] == 0
    p = SC.planted(mode, rng, K, 0 if mode == 1 else -1, 2, K + 8, K + 8)
    assert f(p["a"], p["b"], K)["weak"] == 0
    m = f(p["a"], p["b"], K, force_weak=1)
    assert (m["shift"], m["rot"], m["weak"]) == (0, 0, 1) and m["raw_rot"] == 2


def test_tie_order_and_the_weak_boundary():
    K = 32
    c = np.tile((50, 0), (K + 8, 1))
    for f in (R.match_tails, R.match_heads):
        m = f(c, c, K)                                              # every shift scores the same: 0 comes first
        assert len({s[1] for s in m["scores"]}) == 1 and (m["shift"], m["rot"], m["weak"]) == (0, 0, 0)
        m = f(c, np.tile((50, -50), (K + 8, 1)), K)                 # re == im: rotation 0 before 1
        assert m["scores"][0][1] == m["scores"][0][2] > 0 and m["rot"] == 0
        m = f(c, np.tile((-50, -50), (K + 8, 1)), K)                # im == -re > 0: rotation 1 before 2
        assert m["rot"] == 1
    m = R.match_rails(np.tile((50, 50), (K + 8, 1)), np.tile((-50, 0), (K + 8, 1)), K)
    assert m["tots"][2] == m["tots"][3] == max(m["tots"]) and m["rot"] == 2
    for mode in range(3):
        kinds = {}
        for p in SC.seam_batch(mode, K):
            kinds.setdefault(p["kind"], []).append(MATCH[mode](p["a"], p["b"], K))
        assert all(4 * m["best"] ** 2 == m["ea"] * m["eb"] and m["best"] > 0 and not m["weak"] for m in kinds["boundary"])
        assert all(m["ea"] * m["eb"] - 4 * m["best"] ** 2 == m["eb"] and m["weak"] for m in kinds["boundary_below"])


def test_assemble_and_window_power_models():
    src = np.array([[1, 2], [-128, 127], [3, -4], [5, 6], [-7, 8]], dtype=np.int8)
    out = np.full((8, 2), 90, dtype=np.int8)
    R.assemble(out, src, [1, 0], [2, 1], [1, 2], [-1, 4], [0, 3], [1, 4])
    # tile 0: (-128 + 127j) * j = -127 - 128j; (3 - 4j) * j = 4 + 3j.  tile 1: head (-7 + 8j) * -j = 8 + 7j, then -(1 + 2j)
    assert out.tolist() == [[90, 90], [-127, -128], [4, 3], [90, 90], [8, 7], [-1, -2], [90, 90], [90, 90]]
    out2 = np.full((2, 2), 90, dtype=np.int8)
    R.assemble(out2, src, [1], [1], [2], [-1], [0], [0])
    assert out2[0].tolist() == [-128, -127]                          # -(-128) wraps to -128
    assert R.window_power(src, 0, 0) == 0.0 and R.window_power(src, 3, 1) == 0.0
    u8 = np.array([[128, 128], [130, 128], [126, 128]], dtype=np.uint8)
    assert R.window_power(u8, 0, 3) == pytest.approx(8.0 / 3.0)
    f = np.array([[1000.0, -1000.0], [1001.0, -1000.0]], dtype=np.float32)
    assert R.window_power(f, 0, 2) == pytest.approx(0.25)


def test_carrier_model_finds_a_noiseless_tone():
    """z = A exp(2 pi j f n): the 4th-power line sits at 4 f nwin bins; found to 0.01 bin at every geometry of the GPU cases."""
    for name, (fs, sr, oq, bps, window, (decim, pre), *_rest) in SC.CARRIER_CASES.items():
        nwin, d, l2, kmax, p = R.carrier_geometry(fs, sr, window)
        assert (d, p) == (decim, pre), name
        for bins in (37.3, -12.75, 101.45):       # (a tone of a cycle or so per window is partly mean, and the mean removal bends it)
            n = np.arange(nwin + 100)
            z = 1000.0 * np.exp(2j * np.pi * (bins / 4.0 / nwin) * n + 0.3j)
            iq = np.stack((z.real, z.imag), axis=1).astype(np.float32)
            e = R.carrier_estimate(iq, fs, sr, oq, [7], window)[0]
            assert abs(e["k"] + e["delta"] - bins) < 0.01, (name, bins, e)
            rad_per_bin = 2 * math.pi * (fs / 4.0 / nwin) / (sr * (2 if oq else 1))          # carrier rad per NCO step, per bin of z^4
            assert abs(e["freq"] - bins * rad_per_bin) < 0.01 * rad_per_bin


@pytest.mark.parametrize("oqpsk,bps,ppm", [(False, 16, 7.3), (False, 8, -150.0), (True, 16, 31.0), (True, 32, -12.0)])
def test_clock_model_finds_the_generators_rate(oqpsk, bps, ppm):
    symrate = 80000 if oqpsk else 72000
    cfg = DemodConfig(samplerate=230000, symrate=symrate, oqpsk=oqpsk, bps=bps)
    f0 = 900.0
    st = synth.make_stream(71, 230000, symrate, f0_hz=f0, clock_ppm=ppm, esn0_db=12.0, oqpsk=oqpsk, fmt=bps, **SC.AMP[bps])
    iq = synth.generate_host(st, 200_000)
    starts = [0, 100_001]
    fc = np.full(2, 2 * np.pi * f0 / (symrate * (2 if oqpsk else 1)), dtype=np.float32)
    est = R.clock_estimate(iq, 230000, symrate, oqpsk, cfg.interp_factor, starts, 70_000, carrier=fc if oqpsk else None)
    true = 2 * np.pi * (st.sym_step / 2.0 ** 32) / cfg.interp_factor
    for e in est:
        assert e["nwin"] == 65536 and abs(e["t_freq"] / true - 1) < 3e-6, e
        assert e["quality"] > 15


def test_window_geometry_is_the_librarys():
    lib = _capi.lib()
    for fs, sr, oq, bps, window, *_rest in list(SC.CARRIER_CASES.values()) + [(230000, 72000, False, 16, w) for w in (100, 5000, 100_000, 1 << 20)]:
        p = DemodConfig(samplerate=fs, symrate=sr, oqpsk=oq, bps=bps).to_c()
        assert R.carrier_geometry(fs, sr, window)[0] == lib.mdemod_carrier_window_samples(C.byref(p), window), (fs, sr, window)
    for name, (fs, sr, oq, bps, window, decim, *_rest) in SC.CLOCK_CASES.items():
        assert R.clock_geometry(fs, sr, oq, window)[:2] == (window, decim), name
