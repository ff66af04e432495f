"""The std window's FIR padding bounds (csrc/rot_fir_bounds.h: rot_fir_q, rot_fir_flags; used by WinF::fir in
csrc/demod_kernel_rot.hip) on the host: no device needed.

The kernel votes with three lane masks (a >= 4, a >= 8, a >= 12 over the lanes of the firing) where it used to bisect with four
votes.  The header is compiled into a small stand-alone program that walks every pair of smallest / largest alignment a wave can
have (0 <= a_min <= a_max <= 15: 136 pairs), builds the masks a wave with those alignments produces under several exec masks with
lanes switched off, and checks
  * the flags against the expression they replace, ((1 << q_lo) - 1) | (((1 << (3 - q_hi)) - 1) << 3) with q_lo = a_min / 4 and
    q_hi = a_max / 4 taken from the lanes directly,
  * that no half-chunk of 4 slots that holds a tap of an active lane (slots a .. a + 64) is flagged as padding."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "meteor_demod_amd" / "csrc"

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "rot_fir_bounds.h"

/* the functions are usable in constant expressions */
static_assert(rot_fir_flags(0, 3) == 0 && rot_fir_flags(3, 3) == 7 && rot_fir_flags(0, 0) == 0x38 && rot_fir_flags(1, 2) == (1 | 8), "flags");
static_assert(rot_fir_q(~0ull, ~0ull, 0, 0).q_lo == 1 && rot_fir_q(~0ull, ~0ull, 1, 0).q_hi == 2, "masks");

static const uint64_t EXECS[] = { ~0ull, 0x8000000000000001ull, 0x00000000FFFFFFFFull, 0xAAAAAAAAAAAAAAAAull, 0x0000000000000003ull,
                                  0x0123456789ABCDEFull, 0x0000000000010000ull, 0x7FFFFFFFFFFFFFFEull };

int main()
{
	int pairs = 0, cases = 0, bad = 0;
	for (int a_min = 0; a_min <= 15; a_min++)
		for (int a_max = a_min; a_max <= 15; a_max++) {
			pairs++;
			for (unsigned e = 0; e < sizeof(EXECS) / sizeof(EXECS[0]); e++) {
				const uint64_t ex = EXECS[e];
				/* alignments of the 64 lanes: the first active lane has a_min, the last a_max, the others something in between;
				   lanes that are off carry alignments OUTSIDE the range, which must not count */
				int a[64], first = -1, last = -1, n_active = 0;
				for (int l = 0; l < 64; l++) if (ex >> l & 1) { if (first < 0) first = l; last = l; n_active++; }
				if (n_active == 1 && a_min != a_max) continue;                 /* one lane has one alignment */
				for (int l = 0; l < 64; l++) {
					if (!(ex >> l & 1)) a[l] = (l & 1) ? 0 : 15;
					else a[l] = a_min + (int)(((unsigned)l * 2654435761u >> 7) % (unsigned)(a_max - a_min + 1));
				}
				a[first] = a_min; a[last] = a_max;
				uint64_t m4 = 0, m8 = 0, m12 = 0;
				for (int l = 0; l < 64; l++) if (ex >> l & 1) {                /* a v_cmp writes the bits of active lanes only */
					if (a[l] >= 4) m4 |= 1ull << l;
					if (a[l] >= 8) m8 |= 1ull << l;
					if (a[l] >= 12) m12 |= 1ull << l;
				}
				const RotFirQ q = rot_fir_q(ex, m4, m8, m12);
				const int flags = rot_fir_flags(q.q_lo, q.q_hi);
				const int q_lo = a_min / 4, q_hi = a_max / 4;
				const int want = ((1 << q_lo) - 1) | (((1 << (3 - q_hi)) - 1) << 3);
				cases++;
				if (q.q_lo != q_lo || q.q_hi != q_hi || flags != want) {
					printf("a_min %d a_max %d exec %016llx: q %d %d flags %02x, want q %d %d flags %02x\n", a_min, a_max,
					       (unsigned long long)ex, q.q_lo, q.q_hi, flags, q_lo, q_hi, want);
					bad++;
				}
				/* half-chunk h = slots 4h .. 4h + 3; bit b < 3 flags half-chunk b, bit 3, 4, 5 everything from half-chunk 19, 18, 17 on */
				for (int l = 0; l < 64; l++) if (ex >> l & 1)
					for (int h = 0; h < 20; h++) {
						const bool has_tap = 4 * h + 3 >= a[l] && 4 * h <= a[l] + 64;
						const bool flagged = (h < 3 && (flags >> h & 1)) || (h >= 19 && (flags >> 3 & 1)) ||
						                     (h >= 18 && (flags >> 4 & 1)) || (h >= 17 && (flags >> 5 & 1));
						if (has_tap && flagged) { printf("a %d (lane %d): half-chunk %d holds a tap and is flagged (%02x)\n", a[l], l, h, flags); bad++; }
					}
			}
		}
	printf("pairs %d cases %d bad %d\n", pairs, cases, bad);
	return bad ? 1 : 0;
}
"""


def test_three_masks_give_the_flags_of_the_bisection_and_skip_no_tap(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "rot_fir_bounds_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rot_fir_bounds_check"
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-4000:]
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[0] == "pairs" and int(last[1]) == 136 and int(last[3]) >= 136 * 6 and int(last[5]) == 0, run.stdout[-400:]
