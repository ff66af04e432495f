"""CPU tests of the helpers behind tests/test_gpu_frontend_exact.py: the expected impulse outputs against a float64 convolution,
the branches of fe_plan that the ten geometries reach, the tap coverage and the call cuts of every case, and the float32
restatement of the mixer against float64.  No GPU is touched."""
from __future__ import annotations

import numpy as np
import pytest

import frontend_util as U


def test_expected_impulse_outputs_are_a_float64_convolution_rounded_once():
    """D = 5, 16 taps per phase, all three formats: np.convolve in float64 of the converted input with the float taps, every
    D-th output, rounded to float32 - the helper's np.float32(h[k]) * np.float32(a) and zeros, value for value."""
    d, tpp = 5, 16
    h = U.taps(d, tpp)
    for bps in (8, 16, 32):
        tr = U.impulse_train(d, len(h), bps, seed=bps)
        z = U.to_complex(tr.x, bps)
        y = np.convolve(z, h.astype(np.float64))[: tr.n][::d]
        want = np.stack([y.real, y.imag], axis=1).astype(np.float32)
        got = U.expected(tr, h)
        assert got.shape == (-(-tr.n // d), 2) and got.dtype == np.float32
        assert np.array_equal(got, want), bps
        assert np.count_nonzero(got[:, 0]) == len(h)            # every tap once: D responses of L / D outputs each, about
        # a shorter count cuts the outputs, not their values
        n = int(tr.at[2]) + 7
        assert np.array_equal(U.expected(tr, h, n), want[: -(-n // d)])
        # and the two float models agree with it on this input (products with zeros only)
        for dtype in (np.complex128, np.complex64):
            m = U.filter_model(z, h, d, dtype)
            assert np.array_equal(np.stack([m.real, m.imag], axis=1).astype(np.float32), want), (bps, dtype)


def test_plan_arithmetic_reaches_every_branch():
    """Each geometry reaches the branch the table names, from FE_BLOCK and FE_SPAN_MAX as the source defines them; between them:
    4, 2 and 1 outputs per thread, G = 2, 4, 8 and 16, and a shared-output case whose last thread has no phase."""
    c = U.source_constants()
    assert c["FE_BLOCK"] == 256, c
    seen = set()
    empty_last = short_before_last = False
    for d, tpp, want in U.GEOMETRIES:
        p = U.plan(d, tpp)
        assert p["span"] <= c["FE_SPAN_MAX"] and p["L"] == U.n_taps(d, tpp)
        assert U.branch(d, tpp) == want, (d, tpp, U.branch(d, tpp))
        seen.add(want)
        lo_hi = p["ranges"]
        assert sorted(r for lo, hi in lo_hi for r in range(lo, hi)) == list(range(d))          # every phase once
        if p["G"] > 1 and lo_hi[-1][0] == lo_hi[-1][1]:
            empty_last = True
            short_before_last = 0 < lo_hi[-2][1] - lo_hi[-2][0] < p["per"]
    assert {("R", 4), ("R", 2), ("R", 1), ("G", 2), ("G", 4), ("G", 8), ("G", 16)} <= seen, seen
    assert empty_last and short_before_last
    p = U.plan(65, 16)
    assert p["per"] == 17 and p["ranges"][-1] == (51, 65)
    p = U.plan(100, 32)
    assert p["per"] == 7 and p["ranges"][14] == (98, 100) and p["ranges"][15] == (105, 105)
    assert U.plan(128, 32)["T"] == 16


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_every_tap_is_hit_and_the_cuts_cut_a_response(case):
    d, tpp = case
    L = U.n_taps(d, tpp)
    for bps in (8, 16, 32):
        tr = U.impulse_train(d, L, bps, seed=1)
        assert len(tr.at) == d and sorted(tr.at % d) == list(range(d))
        assert np.all(np.diff(tr.at) >= L + d) and tr.at[-1] + L <= tr.n
        assert d == 1 or tr.n % d != 0
        assert U.taps_hit(tr) == set(range(L))
        x = U.to_complex(tr.x, bps)
        assert np.count_nonzero(x) == d
        if bps == 16 and d >= 2:
            assert {1, -1, 32767, -32768} <= set(tr.x[tr.at].reshape(-1).tolist())
        if bps == 8 and d >= 2:
            assert {0, 255} <= set(tr.x[tr.at].reshape(-1).tolist())
    calls = U.cuts_for(tr)
    assert sum(calls) == tr.n and len(calls) <= 300
    if L > 2:
        assert U.cut_properties(calls, tr.at, L) == (True, True)
    sizes = set(U.cut_sizes(d, L - 1))
    assert all(k in sizes for k in calls[:-1])


def test_float32_mixer_restatement_against_float64():
    """The numbers of the mixer-alone test: fs = 1 MS/s, offset 123 456.7 Hz, 2^21 samples of (12345, -7001).  All 1024 entries of
    both tables occur, and the float32 restatement of fe_mix is within 4e-6 |x| of the float64 rotation (3.11e-6 measured): the
    bar of the GPU test leaves room for the arithmetic it describes."""
    from meteor_demod_amd.frontend import phase_step
    step = phase_step(123456.7, 1000000)
    n = 1 << 21
    hi, lo = U.table_indices(U.phase_words(step, n))
    assert set(hi.tolist()) == set(range(1024)) and set(lo.tolist()) == set(range(1024))
    z = np.full(n, 12345.0 - 7001.0j)
    err = np.abs(U.mix32(z, step).astype(np.complex128) - U.mix64(z, step)).max() / abs(z[0])
    print(f"mix32 against mix64: {err:.3e} of |x|")
    assert err <= 4e-6
    # the index is absolute: a piece from n0 is that piece of the whole
    assert np.array_equal(U.mix32(z[:1000], step, n0=777), U.mix32(z[:1777], step)[777:])
    assert np.array_equal(U.mix64(z[:1000], step, n0=777), U.mix64(z[:1777], step)[777:])
