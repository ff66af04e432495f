"""CPU: the compiler-generated vector instructions of a firing's scalar stage in the configs[1] instance of the std rotating-window
kernel, `demod_kernel_rot<16, 0, 14, 0, 1>` - from the `s_setprio 2` behind the FIR to the `s_setprio 0`, read from the device assembly
build() keeps next to the objects (as tests/test_rot_state_regs.py reads it) - against the count of the commit before round 11.

Round 11 (profiles/r11_firing_bookkeeping.md) took seven of them out of the span: three of the output ring's eight (the byte offset is
stepped, not recomputed from the symbol count), two of the clock table's six index instructions (a select cascade and one three-way
addition), the symbol counter's increment and the copy of it in front of the ring write (the ring counts the symbols).  Two more
copies left the loop's tail behind the `s_setprio 0` (the sample position advances in place), which keeps one: t_prev <- out_im."""
from __future__ import annotations

from test_rot_state_regs import _rot_kernels

# span of c7fe95cc4abea8efc59514d9b48fbdf371a3d680 (the parent of round 11), counted by this file's rule from that commit's assembly
PARENT_SPAN_VALU = 168
PARENT_TAIL_VALU = 3
REMOVED_FROM_SPAN = 7
REMOVED_FROM_TAIL = 2


def _configs1():
    (ins,) = [v[0] for k, v in _rot_kernels().items() if "demod_kernel_rotILi16ELi0ELi14ELi0ELi1EE" in k]
    first, last = [ins.index(t) for t in ("s_setprio 2", "s_setprio 0")]
    assert ins.count("s_setprio 2") == 1 and ins.count("s_setprio 0") == 1 and first < last
    return ins, first, last


def test_scalar_stage_of_configs1_lost_the_bookkeeping_instructions():
    ins, first, last = _configs1()
    valu = [t for t in ins[first + 1:last] if t.startswith("v_")]
    assert len(valu) <= PARENT_SPAN_VALU - REMOVED_FROM_SPAN, len(valu)
    # what went: no shift builds the ring's or the table's offset any more, and the selects of the table's index have constants only
    assert not [t for t in valu if t.startswith("v_lshlrev_b32") and t.split(",")[1].strip() in ("6", "10")], valu
    assert len([t for t in valu if t.startswith("v_add3_u32")]) <= 1, valu


def test_loop_tail_of_configs1_keeps_one_copy():
    ins, _, last = _configs1()
    tail = []
    for t in ins[last + 1:]:
        if t.startswith(("s_cbranch", "s_branch")):
            break
        tail.append(t)
    valu = [t for t in tail if t.startswith("v_")]
    assert len(valu) <= PARENT_TAIL_VALU - REMOVED_FROM_TAIL, valu
