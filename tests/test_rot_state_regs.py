"""CPU: the std rotating-window kernels keep four words of the per-firing loop state (err, t_prev, the flag word, the sample index
of the last symbol) in VGPRs (W::REGSLOTS, csrc/demod_kernel_rot.hip) - read from the device assembly build() keeps next to the
objects, as tests/test_host_logic.py reads it for the register partition.

Every `demod_kernel_rot<...>` instance must still have no scratch, two waves per SIMD and the whole VGPR file (the top of it belongs
to the window's assembly).  In the configs[1] instance `<16, 0, 14, 0, 1>` the scalar stage of a firing - the compiler's
instructions from the `s_setprio 2` behind the FIR to the `s_setprio 0` - is left with at most six LDS instructions (the two
sine-table reads, the clock table's entry, the tanh table's two reads and the output ring's write; twelve with the four words in LDS
slots), and none of them is the ds_read2st64 / ds_write2st64 pair that served S_ERR / S_FLAGS."""
from __future__ import annotations

import re

from meteor_demod_amd import build as B


def _rot_kernels() -> dict:
    """mangled name -> (instructions outside inline assembly, metadata comment block) of every demod_kernel_rot<...> instance"""
    path = B.LIB / "demod_kernel_rot.gfx950.s"
    if not path.exists():
        B.build()
    lines = path.read_text().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w*demod_kernel_rotILi\w+):", lines[i])
        if not m:
            i += 1
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        ins, inasm = [], False
        for line in lines[i:end]:
            if "#ASMSTART" in line:
                inasm = True
            elif "#ASMEND" in line:
                inasm = False
            elif not inasm:
                t = line.split(";")[0].strip()
                if t and not t.startswith(".") and not t.endswith(":"):
                    ins.append(t)
        out[m.group(1)] = (ins, "\n".join(lines[end:end + 80]))
        i = end
    return out


def test_every_std_window_instance_keeps_its_resources():
    kernels = _rot_kernels()
    assert len(kernels) == 18, sorted(kernels)             # s16 / u8 / f32 x QPSK / OQPSK x { generic, compact, sine table + compiled-in steps }
    for name, (_, meta) in kernels.items():
        got = {k: int(re.search(k + r":\s*(\d+)", meta).group(1)) for k in ("ScratchSize", "Occupancy", "NumVgprs")}
        assert got == {"ScratchSize": 0, "Occupancy": 2, "NumVgprs": 256}, (name, got)


def test_scalar_stage_of_configs1_has_no_lds_traffic_for_the_moved_words():
    (ins,) = [v[0] for k, v in _rot_kernels().items() if "demod_kernel_rotILi16ELi0ELi14ELi0ELi1EE" in k]
    first, last = [ins.index(t) for t in ("s_setprio 2", "s_setprio 0")]
    assert ins.count("s_setprio 2") == 1 and ins.count("s_setprio 0") == 1 and first < last
    lds = [t for t in ins[first + 1:last] if t.startswith("ds_")]
    assert len(lds) <= 6, lds
    # S_ERR / S_FLAGS were the only users of the two-slot forms; S_TPREV and S_LASTV were written back with plain 4-byte writes: the
    # only write left is the ring's 2-byte one
    assert not [t for t in lds if "read2" in t or "write2" in t], lds
    assert not [t for t in lds if t.startswith("ds_write_b32")], lds
