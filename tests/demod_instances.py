"""The demodulator's kernel instances as a test matrix: ONE ROW PER COMPILED INSTANCE, shared by tests/test_demod_instances_host.py
(CPU: every instance has a row, every row plans to its instance, every row's signal locks, unlocks and relocks in the oracle) and
tests/test_gpu_demod_instances.py (GPU: every row bit-exact against the oracle through lock, unlock and relock).

A row names a configuration and an environment that make mdemod_create pick exactly that instance.  Which instance a context
launches is decided in two places: plan_context / pick_launch (csrc/demod_api.cpp: the launch function and its arguments) and the
launch function of the kernel's file (the template arguments).  `mdemod_plan_launch` (csrc/mdemod_internal_api.h, host only)
reports the first; `instance_label` below restates the second, table by table, and the completeness test holds its labels against
the entry labels of the device assembly build() keeps (lib/*.gfx950.s).  A new `demod_kernel*` instance therefore fails
test_every_compiled_instance_has_exactly_one_row until it has a row here.

The signal of a row is the `c1_fade` pattern of tests/golden_cases.py on the row's configuration: signal at Es/N0 = 20 dB, noise
only (rms 1.0, Es/N0 = -30 dB), signal again - five streams that differ in seed, carrier offset, clock error and segment lengths.
The GPU does not run the lead-in: the oracle does, and its loop state and filter history go into the context through
mdemod_set_state / mdemod_set_history right before a window of +-WINDOW symbols around a transition.  That the device generator
gives the host generator's samples at n0 != 0 is held by tests/test_gpu_synth.py::test_device_equals_host_bit_for_bit."""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field

import numpy as np

import oracle_py as O
from meteor_demod_amd import DemodConfig, _capi, synth
from meteor_demod_amd import build as B

LANES = 70                       # more than a wave, and no multiple of anything
N_STREAMS = 5
KINDS = ("lock", "unlock", "relock", "control")
WINDOW = 256                     # symbols either side of a transition
CHAIN = (1, 3, 64)               # samples of the first calls of a window; the rest goes in as one more call

LANE = {"MDEMOD_LAT": "0"}                                # the lane-per-stream kernels (70 streams alone would take the wave kernel)
V1 = {"MDEMOD_LAT": "0", "MDEMOD_KERNEL": "v1"}           # the LDS ring kernel
WAVE = {"MDEMOD_LAT": "1"}                                # the wave-per-stream (latency) kernel

# words of mdemod_plan_launch (csrc/mdemod_internal_api.h)
(P_KIND, P_BPS, P_OQPSK, P_STEPS, P_SINLUT, P_CLOCKTAB, P_GEOM, P_SLIDES, P_COMPACT, P_LONG, P_V1_BLOCK, P_V1_GTAB, P_V1_NGW,
 P_FLOAT_HIST) = range(14)
K_LAT, K_GAT, K_ROTH, K_ROT, K_ROTP, K_V1 = range(6)


@dataclass(frozen=True)
class Signal:
    """Levels (complex rms in LSB of the sample format) and segment lengths in symbols (signal, noise only, signal) of a row's clips.
    Stream k adds k * stagger symbols to every segment, so that the transitions the segment borders cause fall at different symbols."""
    rms: float
    noise_rms: float = 1.0       # of the noise-only segment (Es/N0 = -30 dB)
    spread: tuple = (1.0, 1.0, 1.0, 1.0, 1.0)                 # signal level of stream k = rms * spread[k]
    segs: tuple = (7000, 3000, 7000)
    stagger: int = 173
    f0_hz: tuple = (-40.0, 20.0, 70.0, 120.0, 170.0)          # within +-300 Hz: the PLL's sweep (1e-6 rad per symbol) is no help here
    clock_ppm: tuple = (-40.0, 25.0, -10.0, 40.0, 5.0)


@dataclass(frozen=True)
class Row:
    label: str                   # the instance, template arguments spelled out as the device assembly's entry label has them
    cfg: DemodConfig
    env: dict
    name: str                    # piece of mdemod_kernel_name
    block: int                   # threads per block
    pin: str                     # the fact that makes the planner pick THIS instance of the family
    signal: Signal
    steps: int | None = None     # blind steps of the planned clock table (tests/test_gpu_clock_table.py: _planned) where they decide the instance
    lead_in: str = "import"      # "import": oracle state and history imported; anything else would say why the GPU runs the lead-in


# ---- signal levels -------------------------------------------------------------------------------------------------------------
# What unlocks a locked loop in this demodulator is an amplitude transient.  Once the AGC (agc.c: gain += 1e-4 * (190 - |y|) per symbol)
# has a signal at its target, pll.c's error average sits at 0.527 * 190 = 100.2 for ANY input of random phase - noise, or a signal
# the loop has lost - below the 105 that unlock.  So a clip unlocks at a segment border, where the level jumps, and only if the AGC
# is slow enough there to let |e| * 1e-3 add up to 20 or so: its relative step per symbol is 1e-4 times the amplitude BEHIND the
# filter, which grows with the samples per symbol (the RRC taps are not normalised).
#   - float input (28 rows) takes the pattern as c1_fade has it: a signal of rms 0.3 or less lies far below the noise segment
#     (rms 1.0 at -30 dB is a sigma of sqrt(500 * samples per symbol)), and the loop unlocks where the noise starts;
#   - s16 and u8 at up to 3.2 samples per symbol (28 rows) take it too: s16 unlocks where the strong signal comes back to a gain
#     the noise has let rise, u8 at rms 4 .. 10 where the noise starts;
#   - s16 and u8 from 6.9 samples per symbol up (29 rows: every packed-window and gather row, the 129-tap ring rows, the generic latency
#     rows) CANNOT unlock on a noise segment of rms 1.0: behind the filter that noise is 22 * samples per symbol, the AGC follows it
#     within 30 symbols at 1 MS/s and within 3 at 10 MS/s, and a signal small enough to sit far below it (rms under 22 / (1 + 0.55 *
#     samples per symbol): 2.5 LSB at 1 MS/s, 0.3 at 10 MS/s) is no signal in an integer format.  These rows generate the noise-only
#     segment at rms 0.01 (still Es/N0 = -30 dB; a sigma of 0.8 .. 2.6 LSB): the gain rises during it, and a healthy signal (rms
#     50 .. 1250) unlocks the loop when it returns.  noise_rms says so in the row.
# Each entry was found with the oracle, by trying a handful of levels in a fixed order (noise at rms 1.0 first) until all five
# streams lock, unlock and relock at pairwise different symbols - the condition
# test_every_row_locks_unlocks_and_relocks_in_the_oracle holds this table to.
SIGNALS = {
    "demod_kernel<16,0,0,2,0>": Signal(rms=8000.0),
    "demod_kernel<16,0,0,2,1>": Signal(rms=4.0),
    "demod_kernel<16,0,17,2,0>": Signal(rms=5008.7),
    "demod_kernel<16,0,33,2,0>": Signal(rms=288.0, noise_rms=0.01),
    "demod_kernel<16,1,0,2,0>": Signal(rms=8000.0),
    "demod_kernel<16,1,0,2,1>": Signal(rms=5565.2),
    "demod_kernel<16,1,17,2,0>": Signal(rms=4.0),
    "demod_kernel<16,1,33,2,0>": Signal(rms=80.0, noise_rms=0.01),
    "demod_kernel<32,0,0,2,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel<32,0,0,2,1>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel<32,0,17,2,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel<32,0,33,2,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel<32,1,0,2,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel<32,1,0,2,1>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel<32,1,17,2,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel<32,1,33,2,0>": Signal(rms=0.03, spread=(1.0, 2.0, 4.0, 8.0, 16.0)),
    "demod_kernel<8,0,0,2,0>": Signal(rms=10.0),
    "demod_kernel<8,0,0,2,1>": Signal(rms=4.0),
    "demod_kernel<8,0,17,2,0>": Signal(rms=4.0),
    "demod_kernel<8,0,33,2,0>": Signal(rms=50.0, noise_rms=0.01, segs=(7000, 8000, 7000)),
    "demod_kernel<8,1,0,2,0>": Signal(rms=4.0),
    "demod_kernel<8,1,0,2,1>": Signal(rms=4.0),
    "demod_kernel<8,1,17,2,0>": Signal(rms=4.0),
    "demod_kernel<8,1,33,2,0>": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_gat<16,0,129>": Signal(rms=288.0, noise_rms=0.01),
    "demod_kernel_gat<16,0,65>": Signal(rms=192.0, noise_rms=0.01),
    "demod_kernel_gat<16,1,129>": Signal(rms=177.8, noise_rms=0.01),
    "demod_kernel_gat<16,1,65>": Signal(rms=160.0, noise_rms=0.01),
    "demod_kernel_gat<32,0,65>": Signal(rms=0.1, spread=(1.0, 2.0, 4.0, 8.0, 16.0)),
    "demod_kernel_gat<32,1,65>": Signal(rms=0.03, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_gat<8,0,129>": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_gat<8,0,65>": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_gat<8,1,129>": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_gat<8,1,65>": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_lat<16,0,0>": Signal(rms=1125.0, noise_rms=0.01),
    "demod_kernel_lat<16,0,14>": Signal(rms=5008.7),
    "demod_kernel_lat<16,1,0>": Signal(rms=1250.0, noise_rms=0.01),
    "demod_kernel_lat<16,1,6>": Signal(rms=4.0),
    "demod_kernel_lat<32,0,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_lat<32,0,14>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_lat<32,1,0>": Signal(rms=0.03, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_lat<32,1,6>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_lat<8,0,0>": Signal(rms=50.0, noise_rms=0.01, segs=(7000, 8000, 7000)),
    "demod_kernel_lat<8,0,14>": Signal(rms=4.0),
    "demod_kernel_lat<8,1,0>": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_lat<8,1,6>": Signal(rms=4.0),
    "demod_kernel_rot<16,0,0,0,0>": Signal(rms=8000.0),
    "demod_kernel_rot<16,0,0,1,0>": Signal(rms=5008.7),
    "demod_kernel_rot<16,0,14,0,1>": Signal(rms=5008.7),
    "demod_kernel_rot<16,1,0,0,0>": Signal(rms=8000.0),
    "demod_kernel_rot<16,1,0,1,0>": Signal(rms=4.0),
    "demod_kernel_rot<16,1,6,0,1>": Signal(rms=4.0),
    "demod_kernel_rot<32,0,0,0,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_rot<32,0,0,1,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_rot<32,0,14,0,1>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_rot<32,1,0,0,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_rot<32,1,0,1,0>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_rot<32,1,6,0,1>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_rot<8,0,0,0,0>": Signal(rms=10.0),
    "demod_kernel_rot<8,0,0,1,0>": Signal(rms=4.0),
    "demod_kernel_rot<8,0,14,0,1>": Signal(rms=4.0),
    "demod_kernel_rot<8,1,0,0,0>": Signal(rms=4.0),
    "demod_kernel_rot<8,1,0,1,0>": Signal(rms=4.0),
    "demod_kernel_rot<8,1,6,0,1>": Signal(rms=4.0),
    "demod_kernel_roth<0,256,10,2>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_roth<0,256,2,2>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_roth<0,256,2,3>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_roth<0,256,5,3>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_roth<1,256,10,2>": Signal(rms=0.03, spread=(1.0, 2.0, 4.0, 8.0, 16.0)),
    "demod_kernel_roth<1,256,2,2>": Signal(rms=0.3, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_roth<1,256,2,3>": Signal(rms=0.03, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_roth<1,256,5,3>": Signal(rms=0.03, spread=(1.0, 1.6, 2.5, 4.0, 6.3)),
    "demod_kernel_rotp_FAR_16_0": Signal(rms=562.5, noise_rms=0.01),
    "demod_kernel_rotp_FAR_16_1": Signal(rms=360.0, noise_rms=0.01),
    "demod_kernel_rotp_FAR_8_0": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_rotp_FAR_8_1": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_rotp_MID_16_0": Signal(rms=1125.0, noise_rms=0.01),
    "demod_kernel_rotp_MID_16_1": Signal(rms=1125.0, noise_rms=0.01),
    "demod_kernel_rotp_MID_8_0": Signal(rms=50.0, noise_rms=0.01, segs=(7000, 8000, 7000)),
    "demod_kernel_rotp_MID_8_1": Signal(rms=50.0, noise_rms=0.01),
    "demod_kernel_rotp_WIDE_16_0": Signal(rms=576.0, noise_rms=0.01),
    "demod_kernel_rotp_WIDE_16_0_ks109": Signal(rms=288.0, noise_rms=0.01),
    "demod_kernel_rotp_WIDE_16_1": Signal(rms=80.0, noise_rms=0.01),
    "demod_kernel_rotp_WIDE_8_0": Signal(rms=50.0, noise_rms=0.01, segs=(7000, 8000, 7000)),
    "demod_kernel_rotp_WIDE_8_1": Signal(rms=50.0, noise_rms=0.01),
}


# ---- the matrix ------------------------------------------------------------------------------------------------------------------

def _cfg(samplerate, bps=16, oqpsk=False, **kw) -> DemodConfig:
    if oqpsk:
        kw.setdefault("symrate", 80000)
    return DemodConfig(samplerate=samplerate, bps=bps, oqpsk=oqpsk, **kw)


def _rows() -> list[Row]:
    rows: list[Row] = []

    def add(label, cfg, env, name, block, pin, steps=None):
        rows.append(Row(label, cfg, env, name, block, pin, SIGNALS[label], steps))

    for f in (16, 8, 32):
        # -- std rotating register window (demod_kernel_rot.hip: launch_rot) --
        name = "v3 rotating register window"
        add(f"demod_kernel_rot<{f},0,14,0,1>", _cfg(230000, f), LANE, name, 512, "block 512 + 14 table steps + sine table: BASELINE configs[1]", 14)
        add(f"demod_kernel_rot<{f},1,6,0,1>", _cfg(230000, f, True), LANE, name, 512, "block 512 + 6 table steps + sine table: BASELINE configs[2]", 6)
        add(f"demod_kernel_rot<{f},0,0,0,0>", _cfg(137000, f, interp_factor=8), LANE, name, 256,
            "block 256: -O 8 leaves no room for the sine table, 14 steps through the generic body", 14)
        add(f"demod_kernel_rot<{f},1,0,0,0>", _cfg(143000, f, True, interp_factor=8), LANE, name, 256,
            "block 256: -O 8 leaves no room for the sine table, 6 steps through the generic body", 6)
        add(f"demod_kernel_rot<{f},0,0,1,0>", _cfg(230000, f, interp_factor=20), LANE, name, 256, "-O 20: sixteen rows per bank pass 100 KB, compact rows")
        add(f"demod_kernel_rot<{f},1,0,1,0>", _cfg(230000, f, True, interp_factor=20), LANE, name, 256, "-O 20: compact rows")
        # -- latency kernel (demod_kernel_lat.hip: launch_lat) --
        name = "demod_kernel_lat"
        add(f"demod_kernel_lat<{f},0,14>", _cfg(230000, f), WAVE, name, 64, "MDEMOD_LAT=1 + 14 blind steps")
        add(f"demod_kernel_lat<{f},1,6>", _cfg(230000, f, True), WAVE, name, 64, "MDEMOD_LAT=1 + 6 blind steps")
        add(f"demod_kernel_lat<{f},0,0>", _cfg(1024000, f), WAVE, name, 64, "MDEMOD_LAT=1 + 69 blind steps: the generic clock")
        add(f"demod_kernel_lat<{f},1,0>", _cfg(1024000, f, True), WAVE, name, 64, "MDEMOD_LAT=1 + 30 blind steps: the generic clock")
        # -- v1 LDS ring (demod_kernel.hip: launch_ngw) --
        name = "v1 LDS ring"
        for q in (0, 1):
            add(f"demod_kernel<{f},{q},17,2,0>", _cfg(230000, f, bool(q)), V1, name, 192, "MDEMOD_KERNEL=v1 + 65 taps: 17 window granules")
            add(f"demod_kernel<{f},{q},33,2,0>", _cfg(1000000, f, bool(q), rrc_order=64, interp_factor=8), V1, name, V1_LONG_BLOCK[f],
                "MDEMOD_KERNEL=v1 + 129 taps: 33 window granules")
            add(f"demod_kernel<{f},{q},0,2,0>", _cfg(144000, f, bool(q), symrate=72000, rrc_order=17, interp_factor=3), V1, name, 192,
                "MDEMOD_KERNEL=v1 + 35 taps: the generic window")
            add(f"demod_kernel<{f},{q},0,2,1>", _cfg(230000, f, bool(q), rrc_order=80, interp_factor=64), V1, name, GTAB_BLOCK[f],
                "MDEMOD_KERNEL=v1 + 161 taps x 64 banks: the table stays in global memory")
        # -- gather (demod_kernel_gat.hip: launch_gat_fmt) --
        name = "v3 gather"
        far = 10000000 if f == 32 else 8000000                   # OQPSK halves the samples per firing: float input leaves the far hybrid window above 54
        add(f"demod_kernel_gat<{f},0,65>", _cfg({16: 6000000, 8: 8000000, 32: 6000000}[f], f), LANE, name, 256, "83+ samples per firing, 65 taps")
        add(f"demod_kernel_gat<{f},1,65>", _cfg(far, f, True), LANE, name, 256, "50+ samples per firing (OQPSK), 65 taps")
        if f != 32:                                                # (float input with the long filter has no gather instance: it goes to the v1 ring)
            add(f"demod_kernel_gat<{f},0,129>", _cfg({16: 4000000, 8: 6000000}[f], f, rrc_order=64, interp_factor={16: 4, 8: 3}[f]), LANE, name, 256,
                "55+ samples per firing, 129 taps")
            add(f"demod_kernel_gat<{f},1,129>", _cfg(7200000, f, True, rrc_order=64, interp_factor=3), LANE, name, 256,
                "45 samples per firing (OQPSK), 129 taps")
    # -- hybrid window, float input (demod_kernel_rot.hip: mdemod_launch_demod_roth) --
    for q in (0, 1):
        oq = bool(q)
        add(f"demod_kernel_roth<{q},256,10,2>", _cfg(1000000, 32, oq, rrc_order=64, interp_factor=8), LANE, "v3 hybrid window: float input, 129 taps", 256,
            "float input, 129 taps")
        add(f"demod_kernel_roth<{q},256,2,2>", _cfg(640000, 32, True, rrc_order=24, interp_factor=4) if oq else _cfg(1024000, 32), LANE, "v3 hybrid window, mid", 256,
            "float input, 65 taps, at most 20 samples per firing")
        add(f"demod_kernel_roth<{q},256,2,3>", _cfg(3600000 if oq else 2048000, 32, oq), LANE, "v3 hybrid window, mid", 256,
            "float input, 65 taps, 20..30 samples per firing: many slides")
        add(f"demod_kernel_roth<{q},256,5,3>", _cfg(7200000, 32, True, rrc_order=20, interp_factor=3) if oq else _cfg(3200000, 32), LANE, "v3 hybrid window, far", 256,
            "float input, 65 taps, 30..54 samples per firing")
    # -- packed windows, s16 / u8 (demod_kernel_rotp.hip: mdemod_launch_demod_rotp) --
    wide, mid, far = ("v3 rotating packed window, " + g for g in ("wide", "mid", "far"))
    add("demod_kernel_rotp_WIDE_16_0_ks109", _cfg(1000000, 16, rrc_order=64, interp_factor=8), LANE, wide, WIDE_BLOCK, "BASELINE configs[3]: 109 blind steps + sine table")
    add("demod_kernel_rotp_WIDE_16_0", _cfg(500000, 16, rrc_order=48, interp_factor=6), LANE, wide, WIDE_BLOCK, "97 taps, no 109 steps")
    add("demod_kernel_rotp_WIDE_16_1", _cfg(1000000, 16, True, rrc_order=64, interp_factor=8), LANE, wide, WIDE_BLOCK, "129 taps, OQPSK")
    add("demod_kernel_rotp_WIDE_8_0", _cfg(1000000, 8, rrc_order=64, interp_factor=8), LANE, wide, WIDE_BLOCK, "129 taps, u8")
    add("demod_kernel_rotp_WIDE_8_1", _cfg(1000000, 8, True, rrc_order=64, interp_factor=8), LANE, wide, WIDE_BLOCK, "129 taps, u8, OQPSK")
    add("demod_kernel_rotp_MID_16_0", _cfg(1024000, 16), LANE, mid, 256, "65 taps at 14.2 samples per firing")
    add("demod_kernel_rotp_MID_16_1", _cfg(1024000, 16, True, symrate=72000), LANE, mid, 256, "65 taps at 7.1 samples per firing, OQPSK")
    add("demod_kernel_rotp_MID_8_0", _cfg(1024000, 8), LANE, mid, 256, "65 taps at 14.2 samples per firing, u8")
    add("demod_kernel_rotp_MID_8_1", _cfg(1024000, 8, True, symrate=72000), LANE, mid, 256, "65 taps at 7.1 samples per firing, u8, OQPSK")
    add("demod_kernel_rotp_FAR_16_0", _cfg(2048000, 16), LANE, far, 256, "65 taps at 28.4 samples per firing")
    add("demod_kernel_rotp_FAR_16_1", _cfg(3200000, 16, True, symrate=72000), LANE, far, 256, "65 taps at 22.2 samples per firing, OQPSK")
    add("demod_kernel_rotp_FAR_8_0", _cfg(2150000, 8, rrc_order=20, interp_factor=3), LANE, far, 256, "41 taps at 29.9 samples per firing, u8")
    add("demod_kernel_rotp_FAR_8_1", _cfg(3200000, 8, True, symrate=72000), LANE, far, 256, "65 taps at 22.2 samples per firing, u8, OQPSK")
    return rows


WIDE_BLOCK = 512
V1_LONG_BLOCK = {16: 192, 8: 192, 32: 64}     # three waves per block unless their rings of float pairs leave the LDS no room
GTAB_BLOCK = {16: 192, 8: 192, 32: 64}
ROWS = _rows()
BY_LABEL = {r.label: r for r in ROWS}


# ---- the planner's side ----------------------------------------------------------------------------------------------------------

def planned(row: Row, ns: int = LANES):
    """(kernel name, threads per block, words of mdemod_plan_launch, blind steps of the planned clock table or None) for the row's
    configuration under the row's environment - host arithmetic only.  The caller has put row.env into the environment."""
    lib = _capi.lib()
    p = row.cfg.to_c(ns, 0)
    name = C.create_string_buffer(256)
    block = C.c_uint32()
    rc = lib.mdemod_plan_kernel(C.byref(p), name, 256, None, C.byref(block))
    assert rc == 0, (row.label, rc, _capi.last_error())
    words = (C.c_int32 * 16)()
    assert lib.mdemod_plan_launch(C.byref(p), words) == 0, row.label
    buf = (C.c_int32 * (64 * 16))()
    n = lib.mdemod_plan_clock_table(C.byref(p), buf, 64 * 4)
    assert n >= 0
    steps = None
    if n:
        dv, _, isub_new, _ = buf[0:4]
        steps = (dv - (isub_new > 0)) * row.cfg.interp_factor + isub_new - 1
    return name.value.decode(), block.value, list(words), steps


def instance_label(w) -> str:
    """The compiled instance the launch functions take for the words of mdemod_plan_launch: their tables, restated."""
    f, q, ks = w[P_BPS], w[P_OQPSK], w[P_STEPS]
    if w[P_KIND] == K_LAT:           # demod_kernel_lat.hip: launch_lat
        return f"demod_kernel_lat<{f},{q},{ks if ks == (6 if q else 14) else 0}>"
    if w[P_KIND] == K_GAT:           # demod_kernel_gat.hip: launch_gat_fmt
        return f"demod_kernel_gat<{f},{q},{129 if w[P_LONG] else 65}>"
    if w[P_KIND] == K_ROTH:          # demod_kernel_rot.hip: mdemod_launch_demod_roth
        na, msl = {(1, 1): (2, 3), (1, 0): (2, 2), (2, 0): (5, 3), (2, 1): (5, 3), (0, 0): (10, 2), (0, 1): (10, 2)}[(w[P_GEOM], w[P_SLIDES])]
        return f"demod_kernel_roth<{q},256,{na},{msl}>"
    if w[P_KIND] == K_ROT:           # demod_kernel_rot.hip: launch_rot
        if w[P_COMPACT]:
            return f"demod_kernel_rot<{f},{q},0,1,0>"
        k = 6 if q else 14
        return f"demod_kernel_rot<{f},{q},{k},0,1>" if w[P_SINLUT] and ks == k and w[P_CLOCKTAB] else f"demod_kernel_rot<{f},{q},0,0,0>"
    if w[P_KIND] == K_ROTP:          # demod_kernel_rotp.hip: mdemod_launch_demod_rotp
        if w[P_GEOM] == 0 and f == 16 and not q and ks == 109 and w[P_SINLUT]:
            return "demod_kernel_rotp_WIDE_16_0_ks109"
        return f"demod_kernel_rotp_{('WIDE', 'MID', 'FAR')[w[P_GEOM]]}_{f}_{q}"
    assert w[P_KIND] == K_V1         # demod_kernel.hip: launch_ngw
    if w[P_V1_GTAB]:
        return f"demod_kernel<{f},{q},0,2,1>"
    return f"demod_kernel<{f},{q},{w[P_V1_NGW] if w[P_V1_NGW] in (17, 33) else 0},2,0>"


def compiled_instances() -> list[str]:
    """Labels of every `demod_kernel*` entry of the device assembly build() keeps, template arguments spelled out.  Entry labels
    only: nothing inside the kernels is read."""
    out = []
    for stem in B.DEMOD_KERNEL_UNITS:
        path = B.LIB / (stem + ".gfx950.s")
        if not path.exists():
            B.build()
        for m in re.finditer(r"^_ZN12_GLOBAL__N_1(\d+)(demod_kernel\w*):", path.read_text(), re.M):
            name, rest = m.group(2)[:int(m.group(1))], m.group(2)[int(m.group(1)):]      # <length><name>, then the template arguments
            t = re.match(r"I((?:Li\d+E)+)E", rest)
            out.append(name + ("<" + ",".join(re.findall(r"Li(\d+)E", t.group(1))) + ">" if t else ""))
    return out


# ---- the signal's side -------------------------------------------------------------------------------------------------------------

def make_streams(row: Row):
    """Per stream the list of (descriptor, samples) segments of its clip."""
    cfg, sg = row.cfg, row.signal
    sps = cfg.samplerate / cfg.symrate
    out = []
    for k in range(N_STREAMS):
        segs = []
        for j, s in enumerate(sg.segs):
            kw = dict(esn0_db=20.0, rms=sg.rms * sg.spread[k]) if j != 1 else dict(rms=sg.noise_rms, esn0_db=-30.0)
            st = synth.make_stream(4400 + 16 * k, cfg.samplerate, cfg.symrate, f0_hz=sg.f0_hz[k], clock_ppm=sg.clock_ppm[k],
                                   oqpsk=cfg.oqpsk, fmt=cfg.bps, **kw)
            segs.append((st, int(round((s + k * sg.stagger) * sps))))
        out.append(segs)
    return out


def clip_host(segs) -> np.ndarray:
    parts, n0 = [], 0
    for st, n in segs:
        parts.append(synth.generate_host(st, n, n0))
        n0 += n
    return np.concatenate(parts)


def clip_device(segs) -> np.ndarray:
    """The same samples from the GPU's generator (bit-identical: test_device_generator_equals_host_generator), as a host array."""
    import torch
    parts, n0 = [], 0
    for st, n in segs:
        parts.append(synth.generate_device([st], n, n0=n0)[0])
        n0 += n
    return torch.cat(parts).cpu().numpy()


def decode(iq: np.ndarray) -> np.ndarray:
    """wavfile.c:58-69: the floats the filter sees."""
    return iq.astype(np.float32) - np.float32(128 if iq.dtype == np.uint8 else 0)


@dataclass
class Window:
    stream: int
    kind: str
    event: tuple | None          # (symbol, locked) the window is about; None for the control window
    a: int                       # first sample
    b: int                       # one past the last sample
    # filled by expect()
    state: object = None         # OrcState fields at sample a, as a dict
    history: np.ndarray = None   # the oracle's last `taps` input samples at sample a
    calls: list = field(default_factory=list)     # per chained call: (soft, events)
    final: dict = None           # state after the window
    final_history: np.ndarray = None


def transitions(events):
    """(first lock, the unlock after it, the lock after that) of an oracle event list, None where there is none."""
    lock = next((e for e in events if e[1] == 1), None)
    unlock = next((e for e in events if lock and e[1] == 0 and e[0] > lock[0]), None)
    relock = next((e for e in events if unlock and e[1] == 1 and e[0] > unlock[0]), None)
    return lock, unlock, relock


def find_windows(cfg, k: int, iq: np.ndarray, window: int = WINDOW):
    """One oracle run over the whole clip with a trace: the event list, and the four windows of stream k (None where the clip has
    no such transition, or a window would leave the clip)."""
    soft, trace, events = O.OracleStream(cfg).run(iq, want_trace=True)
    at = trace["sample_index"]
    m = len(soft)

    def win(kind, ev, centre):
        if centre - window < 0 or centre + window >= m:
            return None
        return Window(k, kind, ev, int(at[centre - window]), int(at[centre + window]))

    out = [win(kind, ev, ev[0]) if ev else None for kind, ev in zip(KINDS, transitions(events))]
    # control: the middle of the widest stretch without a transition
    marks = [0] + [e[0] for e in events] + [m - 1]
    gap, lo = max((marks[i + 1] - marks[i], marks[i]) for i in range(len(marks) - 1))
    out.append(win("control", None, lo + gap // 2) if gap > 2 * window + 2 else None)
    return events, out


_STATE_FIELDS = ("gain", "pll_phase", "pll_freq", "pll_err", "locked", "locked_once", "updown", "t_phase", "t_freq", "t_prev", "dual_state",
                 "inphase", "n_samples", "n_symbols", "first_lock_symbol")


def _snapshot(ost) -> dict:
    s = ost.state
    d = {f: getattr(s, f) for f in _STATE_FIELDS}
    d["bias_re"], d["bias_im"] = s.bias.re, s.bias.im
    return d


def chain_lengths(n: int) -> list[int]:
    return list(CHAIN) + [n - sum(CHAIN)]


def expect(cfg, iq: np.ndarray, w: Window) -> Window:
    """The oracle in pieces: the lead-in iq[:a], a snapshot of its state and history, then the window call by call."""
    ost = O.OracleStream(cfg)
    ost.run(iq[:w.a])
    w.state = _snapshot(ost)
    w.history = ost.history()
    pos = w.a
    for n in chain_lengths(w.b - w.a):
        soft, _, ev = ost.run(iq[pos:pos + n])
        w.calls.append((soft, ev))
        pos += n
    w.final = _snapshot(ost)
    w.final_history = ost.history()
    return w


def to_stream_state(d: dict) -> _capi.MdemodStreamState:
    return _capi.MdemodStreamState(d["gain"], d["bias_re"], d["bias_im"], d["pll_phase"], d["pll_freq"], d["pll_err"], d["locked"], d["locked_once"],
                                   d["updown"], d["t_phase"], d["t_freq"], d["t_prev"], d["dual_state"], d["inphase"], d["n_samples"],
                                   d["n_symbols"], d["first_lock_symbol"])
