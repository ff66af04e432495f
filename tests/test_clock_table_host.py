"""The symbol clock's position table (csrc/demod_host.cpp: mdemod_clock_table; read by rot_clock_fast in csrc/rotwin_body.h) against
the arithmetic it replaces, on the host: no device needed."""
from __future__ import annotations

import ctypes as C

import pytest

from meteor_demod_amd import DemodConfig, _capi


def _arithmetic(interp: int, magic: int, k_safe: int, isub: int, j: int) -> tuple[int, int, int, int]:
    """The tail of rot_clock_fast as it was before the table, in Python integers: m = k_safe + 1 + j steps from phase isub, the
    division by -O as __umulhi(w, magic) (32 x 32 -> upper 32 bits; -O 1 skips it: its magic does not fit 32 bits)."""
    w = (isub + k_safe + 1 + j) & 0xFFFFFFFF
    q = w if interp == 1 else ((w * magic) >> 32) & 0xFFFFFFFF
    isub_new = (w - q * interp) & 0xFFFFFFFF
    if isub_new >= 1 << 31:
        isub_new -= 1 << 32
    dv = q + (1 if isub_new > 0 else 0) - (1 if isub > 0 else 0)
    fire_sub = interp - 1 if isub_new == 0 else isub_new - 1
    return dv, fire_sub, isub_new, interp - 1 - fire_sub                      # bank: filter.c:52


def test_every_entry_equals_the_arithmetic_it_replaces():
    """-O 1..64 x 0..200 blind steps x every phase x every count of checked steps: { dv, fire_sub, isub_new, bank } of the table is
    what the arithmetic gives, with the division done the kernel's way (the host's own magic) - and that division is exact."""
    lib = _capi.lib()
    buf = (C.c_int32 * (64 * 16))()
    for interp in range(1, 65):
        magic = lib.mdemod_clock_interp_magic(interp)
        assert magic == ((1 << 32) // interp + 1) & 0xFFFFFFFF
        for k_safe in range(0, 201):
            assert lib.mdemod_clock_table(interp, k_safe, buf, 4 * interp) == 4 * interp
            got = buf[: 16 * interp]
            want = [x for isub in range(interp) for j in range(4) for x in _arithmetic(interp, magic, k_safe, isub, j)]
            assert got == want, (interp, k_safe)
            if k_safe % 50 == 0:                                               # the plain division, too: w // interp
                for isub in range(interp):
                    for j in range(4):
                        w = isub + k_safe + 1 + j
                        e = got[4 * (isub * 4 + j): 4 * (isub * 4 + j) + 4]
                        assert e[2] == w % interp and e[0] == -(-w // interp) - (isub > 0) and 0 <= e[3] < interp and e[1] + e[3] == interp - 1


def test_no_table_beyond_64_banks_and_short_buffers_are_refused():
    lib = _capi.lib()
    buf = (C.c_int32 * (80 * 16))()
    for interp in (0, -1, 65, 80, 1000):
        assert lib.mdemod_clock_table(interp, 14, buf, 80 * 4) == 0
    assert lib.mdemod_clock_table(5, 14, buf, 19) == _capi.MDEMOD_ERR_PARAM
    assert lib.mdemod_clock_table(5, 14, buf, 20) == 20


def _plan(**kw):
    lib = _capi.lib()
    flags = kw.pop("flags", 0)
    p = DemodConfig(**kw).to_c(100000, 0)
    p.reserved = flags | _capi.MDEMOD_FLAG_LAT_OFF
    buf = (C.c_int32 * (64 * 16))()
    n = lib.mdemod_plan_clock_table(C.byref(p), buf, 64 * 4)
    return n, list(buf[: 4 * max(n, 0)])


def _blind_steps(n, tab):
    interp = n // 4
    dv, _, isub_new, _ = tab[:4]                                               # isub 0, j 0: w = k_safe + 1
    return (dv - (isub_new > 0)) * interp + isub_new - 1


PLANS = {
    # configuration -> (entries, blind steps) of its table; 0 entries: the context keeps the arithmetic
    "configs[1]: 14 compiled-in steps": (dict(samplerate=230000), 20, 14),
    "configs[2]: 6 compiled-in steps": (dict(samplerate=230000, symrate=80000, oqpsk=True), 20, 6),
    "configs[3]: 109 compiled-in steps, closed form": (dict(samplerate=1000000, rrc_order=64, interp_factor=8), 0, None),
    "1.024 MS/s mid, generic": (dict(samplerate=1024000), 20, 69),
    "3.2 MS/s far: jump schedule": (dict(samplerate=3200000), 0, None),
    "6 MS/s gather: jump schedule": (dict(samplerate=6000000), 0, None),
    "6 MS/s gather, schedule switched off": (dict(samplerate=6000000, flags=_capi.MDEMOD_FLAG_NO_CLOCK_JUMP), 20, None),
    "-O 32 on the std window (compact rows)": (dict(samplerate=230000, interp_factor=32), 128, None),
    "-O 64 at 18 kS/s": (dict(samplerate=18000, interp_factor=64), 256, 14),
    "-O 1": (dict(samplerate=230000, interp_factor=1), 4, None),
    "v1 ring kernel": (dict(samplerate=230000, flags=1), 0, None),
    "161 taps: v1 ring kernel": (dict(samplerate=230000, rrc_order=80), 0, None),
}


@pytest.mark.parametrize("case", list(PLANS))
def test_which_contexts_get_a_table(case):
    """A table for the fixed-step clocks of the rotating-window kernels; none for a clock with a jump schedule, for the instance
    with 109 compiled-in steps and for the kernels that have no such clock.  The planned table is mdemod_clock_table's."""
    kw, entries, steps = PLANS[case]
    kw = dict(kw)
    interp = kw.get("interp_factor", 5)
    n, tab = _plan(**kw)
    assert n == entries, (n, entries)
    if n:
        assert n == 4 * interp
        k = _blind_steps(n, tab)
        if steps is not None:
            assert k == steps
        buf = (C.c_int32 * (16 * interp))()
        assert _capi.lib().mdemod_clock_table(interp, k, buf, n) == n and list(buf) == tab


def test_an_interpolation_factor_beyond_64_has_no_context_at_all():
    lib = _capi.lib()
    p = DemodConfig(samplerate=230000, interp_factor=65).to_c(100, 0)
    assert lib.mdemod_plan_clock_table(C.byref(p), None, 0) == _capi.MDEMOD_ERR_PARAM
