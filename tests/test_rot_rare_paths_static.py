"""CPU: the control flow of a firing's scalar stage in the configs[1] instance of the std rotating-window kernel,
`demod_kernel_rot<16, 0, 14, 0, 1>` - from the `s_setprio 2` behind the FIR to the `s_setprio 0`, read from the device assembly build()
keeps next to the objects (as tests/test_rot_state_regs.py reads it) - against the counts of the commit before round 12.

Round 12 (profiles/r12_rare_paths.md) puts a firing's rare events - the short cabsf's fallback, two symbols in one input sample, the
far phase wrap, the lock detector's flag arithmetic and the lock event's record - behind ONE scalar branch on the OR of their lane
masks, repaired in one block laid out of line (W::RARE_ONE_BRANCH, csrc/rotwin_body.h).  Left in the span: the fast clock's exec-masked
block, that one branch, and the ring flush's.  Counted by this rule: the text between the two `s_setprio`; branch = `s_cbranch*` or
`s_branch`."""
from __future__ import annotations

from test_rot_state_regs import _rot_kernels

# span of 6ac30d4 (the parent of round 12), counted by this file's rule from that commit's assembly: the cabsf fallback, `again`, the
# fast clock's exec skip, the far fmod wrap, the lock early-out, `changed`, the ring flush
PARENT_SPAN_BRANCHES = 7
PARENT_SPAN_SAVEEXEC = 4
PARENT_BRANCHES_BETWEEN_SINE_READS_AND_WAIT = 1      # the cabsf fallback's: the scheduler works per basic block
REMOVED_BRANCHES = 4


def _span():
    (ins,) = [v[0] for k, v in _rot_kernels().items() if "demod_kernel_rotILi16ELi0ELi14ELi0ELi1EE" in k]
    first, last = [ins.index(t) for t in ("s_setprio 2", "s_setprio 0")]
    assert ins.count("s_setprio 2") == 1 and ins.count("s_setprio 0") == 1 and first < last
    return ins[first + 1:last]


def _is_branch(t: str) -> bool:
    return t.startswith(("s_cbranch", "s_branch"))


def test_scalar_stage_of_configs1_has_three_branches():
    span = _span()
    branches = [t for t in span if _is_branch(t)]
    assert len(branches) <= PARENT_SPAN_BRANCHES - REMOVED_BRANCHES == 3, branches
    saveexec = [t for t in span if t.startswith("s_and_saveexec_b64")]
    assert len(saveexec) <= 3 < PARENT_SPAN_SAVEEXEC, saveexec
    # the one branch of the rare events is scalar: on the OR of the masks, no exec mask saved for it
    assert len([t for t in branches if t.startswith(("s_cbranch_scc", "s_cbranch_vcc"))]) >= 1, branches


def test_sine_table_reads_and_their_wait_share_a_basic_block():
    span = _span()
    # the sine table lies behind the output rings: its two reads are the span's first two ds_read_b32 (the tanh table's come later)
    reads = [j for j, t in enumerate(span) if t.startswith("ds_read_b32")]
    assert len(reads) == 4, [span[j] for j in reads]
    off = [span[j].split("offset:")[1] for j in reads]
    assert off[0] == off[1] and off[2] == off[3] and off[0] != off[2], off
    wait = next(j for j in range(reads[1] + 1, len(span)) if span[j].startswith("s_waitcnt") and "lgkmcnt" in span[j])
    between = span[reads[0]:wait]
    assert len([t for t in between if _is_branch(t)]) == 0 < PARENT_BRANCHES_BETWEEN_SINE_READS_AND_WAIT, between
