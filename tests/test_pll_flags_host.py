"""The lock detector's flag arithmetic (csrc/pll_flags.h: pll_flags_step, pll_flags_event, pll_flags_locked_after; used by
md_pll_update_packed in csrc/demod_device.h) on the host: no device needed.

The kernel skips pll_flags_step for a whole wave when pll_flags_event is false in every lane.  The header is compiled into a small
stand-alone program that walks every flag word 0..7 x (below, above) in {00, 10, 01} x the frequency inside (-fmax, fmax), at or above
fmax, at or below -fmax, and checks
  * where the event predicate is false: the step returns fl unchanged, first = 0, changed = 0 (so skipping it changes nothing),
  * where it is true: the step equals pll.c:117-128 restated with three ints (locked, locked_once, updown), literally,
  * always: bit 0 of the new flag word is pll_flags_locked_after, the mask the sweep (pll.c:125) takes its condition from."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "meteor_demod_amd" / "csrc"

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "pll_flags.h"

/* the functions are usable in constant expressions */
static_assert(pll_flags_step(0u, 1u, 0u, PLL_FREQ_INSIDE).fl == 3u && pll_flags_step(0u, 1u, 0u, PLL_FREQ_INSIDE).first == 2u, "first lock");
static_assert(pll_flags_step(7u, 0u, 1u, PLL_FREQ_HIGH).fl == 2u && pll_flags_step(7u, 0u, 1u, PLL_FREQ_HIGH).changed == 1u, "unlock and turn");
static_assert(!pll_flags_event(5u, 1u, 0u, PLL_FREQ_INSIDE) && pll_flags_event(5u, 0u, 0u, PLL_FREQ_LOW) && pll_flags_event(4u, 1u, 0u, PLL_FREQ_INSIDE), "event");

int main()
{
	const float fmax = 0.3f;
	/* err for (below, above) = 00, 10, 01; freq (after the sweep, before the clamp) inside, >= fmax, <= -fmax: border values included */
	static const float ERRS[3] = { 95.0f, 84.999f, 105.001f };
	static const float FREQS[3][3] = { { 0.0f, 0.2999f, -0.2999f }, { 0.3f, 0.3000004f, 7.0f }, { -0.3f, -0.3000004f, -7.0f } };
	int cases = 0, events = 0, bad = 0;
	for (uint32_t fl = 0; fl < 8; fl++)
		for (int e = 0; e < 3; e++)
			for (int fc = 0; fc < 3; fc++)
				for (int fv = 0; fv < 3; fv++) {
					const float err = ERRS[e], freq_in = FREQS[fc][fv];
					const uint32_t below = err < 85.0f, above = err > 105.0f;
					const int fcase = freq_in >= fmax ? PLL_FREQ_HIGH : (freq_in <= -fmax ? PLL_FREQ_LOW : PLL_FREQ_INSIDE);
					if (fcase != fc || below != (uint32_t)(e == 1) || above != (uint32_t)(e == 2)) { printf("the table of inputs is wrong\n"); return 2; }

					/* pll.c:117-128, literally, on the reference's three ints */
					int locked = fl & 1, locked_once = fl >> 1 & 1, updown = (fl & 4) ? 1 : -1;
					int first = 0, changed = 0;
					float freq = freq_in;
					if (err < 85 && !locked) {
						locked = 1;
						if (!locked_once) first = 1;
						locked_once = 1;
						changed = 1;
					} else if (err > 105 && locked) {
						locked = 0;
						changed = 1;
					}
					if (freq >= fmax) updown = -1;
					else if (freq <= -fmax) updown = 1;
					const uint32_t want = (uint32_t)locked | (uint32_t)locked_once << 1 | (updown > 0 ? 4u : 0u);

					const bool event = pll_flags_event(fl, below, above, fcase);
					const PllFlagStep s = pll_flags_step(fl, below, above, fcase);
					cases++;
					events += event;
					if (!event && (s.fl != fl || s.first != 0 || s.changed != 0)) {
						printf("fl %u below %u above %u case %d: no event, but the step gives fl %u first %u changed %u\n", fl, below, above, fcase, s.fl, s.first, s.changed);
						bad++;
					}
					if (s.fl != want || (s.first != 0) != (first != 0) || (s.changed != 0) != (changed != 0) || (s.first & ~2u) || (s.changed & ~1u)) {
						printf("fl %u below %u above %u case %d: step fl %u first %u changed %u, pll.c gives fl %u first %d changed %d\n", fl, below, above, fcase,
						       s.fl, s.first, s.changed, want, first, changed);
						bad++;
					}
					if (!event && (want != fl || first || changed)) { printf("fl %u below %u above %u case %d: pll.c changes something without an event\n", fl, below, above, fcase); bad++; }
					if (pll_flags_locked_after(fl, below, above) != (bool)(want & 1u)) { printf("fl %u below %u above %u: locked_after\n", fl, below, above); bad++; }
				}
	printf("cases %d events %d bad %d\n", cases, events, bad);
	return bad ? 1 : 0;
}
"""


def test_flag_step_is_the_identity_without_an_event_and_pll_c_with_one(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "pll_flags_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "pll_flags_check"
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-4000:]
    last = run.stdout.strip().splitlines()[-1].split()
    # 8 flag words x 3 error cases x 3 frequency cases x 3 values each; an event: 8 x 3 x 6 outside (-fmax, fmax), and inside it the
    # 4 unlocked words below 85 and the 4 locked words above 105, x 3 values
    assert last[0] == "cases" and int(last[1]) == 216 and int(last[3]) == 144 + 24 and int(last[5]) == 0, run.stdout[-400:]
