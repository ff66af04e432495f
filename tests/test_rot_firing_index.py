"""A firing's integer bookkeeping (csrc/rot_firing_index.h, used by csrc/rotwin_body.h) on the host: no device needed.

The header is compiled into a small stand-alone program.

Output ring, RING in {16, 32} x BLOCK in {256, 512}: stepping the byte offset from 0 for 3 x RING symbols gives the layout's formula
((k & 7) * 2 + (k >> 3) * BLOCK * 16, written out in the program, not taken from the header) at every k; the offset is 0 after the
step exactly where (k + 1) & (RING - 1) == 0; rot_ring_off of a count equals the formula (what the kernel recomputes after the rare
decrement of "two symbols inside one input sample"), for counts beyond one ring too; rot_ring_count maps every offset back.

Clock table, -O 1, 5 and 8: for every isub and the four monotone (c1, c2, c3) patterns - all-false among them - the select cascade
plus the scaled isub is the sum the kernel formed before, (isub << 6) + 16 * (!c1 + !c2 + !c3); a table of mdemod_clock_table (the
library's own, handed over in a file), copied the way the kernel copies it into LDS (third word scaled), read at that byte offset
gives the entry isub * 4 + j with the third word mapping back to the table's, and following the scaled word through the image walks
the same chain of entries as following the plain one through the table."""
from __future__ import annotations

import ctypes as C
import shutil
import subprocess
from pathlib import Path

from meteor_demod_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "meteor_demod_amd" / "csrc"

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "rot_firing_index.h"

/* usable in constant expressions */
static_assert(rot_ring_step(0u, 32u, 512u) == 2u && rot_ring_step(14u, 32u, 512u) == 8192u && rot_ring_step(14u + 3u * 8192u, 32u, 512u) == 0u, "ring 32 x 512");
static_assert(rot_ring_step(14u + 4096u, 16u, 256u) == 0u && rot_ring_off(9u, 16u, 256u) == 4098u && rot_ring_count(4098u, 256u) == 9u, "ring 16 x 256");
static_assert(rot_clock_sel(true, true, true) == 0u && rot_clock_sel(false, true, true) == 16u && rot_clock_sel(false, false, true) == 32u && rot_clock_sel(false, false, false) == 48u, "cascade");
static_assert(rot_ring_geometry_ok(32u, 512u) && !rot_ring_geometry_ok(64u, 512u) && !rot_ring_geometry_ok(32u, 384u), "geometry");

static int ring(uint32_t RING, uint32_t BLOCK)
{
	int bad = 0;
	uint32_t off = 0;
	for (uint32_t k = 0; k < 3 * RING; k++) {
		const uint32_t kk = k & (RING - 1);
		const uint32_t want = (kk & 7u) * 2u + (kk >> 3) * BLOCK * 16u;       /* rotwin_body.h before the step: stage + (k >> 3) * BLOCK, [k & 7] */
		if (off != want) { printf("ring %u block %u: symbol %u at %u, the layout says %u\n", RING, BLOCK, k, off, want); bad++; }
		if (rot_ring_off(k, RING, BLOCK) != want) { printf("ring %u block %u: rot_ring_off(%u)\n", RING, BLOCK, k); bad++; }
		if (rot_ring_count(want, BLOCK) != kk) { printf("ring %u block %u: rot_ring_count(%u)\n", RING, BLOCK, want); bad++; }
		if (want & rot_ring_gap(BLOCK)) { printf("ring %u block %u: offset %u has gap bits\n", RING, BLOCK, want); bad++; }
		if (rot_ring_step(off, RING, BLOCK) != (((off | rot_ring_gap(BLOCK)) + 2u) & rot_ring_keep(RING, BLOCK))) { printf("ring %u block %u: the OR form differs at %u\n", RING, BLOCK, off); bad++; }
		off = rot_ring_step(off, RING, BLOCK);
		if ((off == 0) != (((k + 1) & (RING - 1)) == 0)) { printf("ring %u block %u: full after symbol %u: %d\n", RING, BLOCK, k, off == 0); bad++; }
		/* the decrement: the count goes back by one from k + 1 and the offset is recomputed - it must be this symbol's again */
		if (rot_ring_off((k + 1) - 1u, RING, BLOCK) != want) bad++;
	}
	return bad;
}

static int clock_table(const char *path, int interp)
{
	int32_t tab[64 * 16], image[64 * 16];
	FILE *f = fopen(path, "rb");
	if (!f || fread(tab, 16, 4 * (size_t)interp, f) != 4 * (size_t)interp) { printf("cannot read %s\n", path); return 1; }
	fclose(f);
	int bad = 0;
	for (int i = 0; i < 4 * interp; i++) {           /* the kernel's copy into LDS */
		memcpy(image + 4 * i, tab + 4 * i, 16);
		image[4 * i + 2] = rot_clock_entry_scaled(tab[4 * i + 2]);
		if (rot_clock_entry_unscaled(image[4 * i + 2]) != tab[4 * i + 2]) { printf("-O %d: entry %d does not map back\n", interp, i); bad++; }
	}
	static const bool PAT[4][3] = { { true, true, true }, { false, true, true }, { false, false, true }, { false, false, false } };
	for (int isub = 0; isub < interp; isub++)
		for (int j = 0; j < 4; j++) {
			const bool c1 = PAT[j][0], c2 = PAT[j][1], c3 = PAT[j][2];
			const uint32_t before = ((uint32_t)isub << 6) + (c1 ? 0u : 16u) + (c2 ? 0u : 16u) + (c3 ? 0u : 16u);
			const uint32_t now = (uint32_t)rot_clock_entry_scaled(isub) + rot_clock_sel(c1, c2, c3);
			if (now != before || now != 16u * (uint32_t)(isub * 4 + j)) { printf("-O %d isub %d j %d: offset %u, before %u\n", interp, isub, j, now, before); bad++; continue; }
			const int32_t *e = image + now / 4, *t = tab + 4 * (isub * 4 + j);
			if (e[0] != t[0] || e[1] != t[1] || e[3] != t[3] || rot_clock_entry_unscaled(e[2]) != t[2]) { printf("-O %d isub %d j %d: the image's entry is not the table's\n", interp, isub, j); bad++; }
		}
	/* a walk: the scaled word through the image, the plain one through the table */
	int32_t s = 0, p = 0;
	for (int step = 0; step < 1000; step++) {
		const int j = (step * 7 + step / 3) & 3;
		s = image[(s + (int32_t)rot_clock_sel(PAT[j][0], PAT[j][1], PAT[j][2])) / 4 + 2];
		p = tab[4 * (p * 4 + j) + 2];
		if (s != rot_clock_entry_scaled(p)) { printf("-O %d: the walks part at step %d\n", interp, step); bad++; break; }
	}
	return bad;
}

int main(int argc, char **argv)
{
	int bad = 0, rings = 0, tables = 0;
	static const uint32_t RINGS[2] = { 16, 32 }, BLOCKS[2] = { 256, 512 };
	for (int r = 0; r < 2; r++)
		for (int b = 0; b < 2; b++) { bad += ring(RINGS[r], BLOCKS[b]); rings++; }
	for (int a = 1; a + 1 < argc; a += 2) { int interp = 0; sscanf(argv[a], "%d", &interp); bad += clock_table(argv[a + 1], interp); tables++; }
	printf("rings %d tables %d bad %d\n", rings, tables, bad);
	return bad ? 1 : 0;
}
"""


def test_ring_step_and_clock_index_equal_the_formulas_they_replace(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "rot_firing_index_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rot_firing_index_check"
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    lib = _capi.lib()
    args = []
    for interp in (1, 5, 8):
        buf = (C.c_int32 * (16 * interp))()
        assert lib.mdemod_clock_table(interp, 14, buf, 4 * interp) == 4 * interp
        path = tmp_path / f"clock_table_O{interp}.bin"
        path.write_bytes(bytes(buf))
        args += [str(interp), str(path)]
    run = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-4000:]
    assert run.stdout.strip().splitlines()[-1] == "rings 4 tables 3 bad 0", run.stdout[-400:]
