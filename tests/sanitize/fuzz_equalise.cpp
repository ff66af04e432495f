/*
 * fuzz_equalise.cpp — the host side of the equalise layer (csrc/equalise_host.cpp) under ASan + UBSan (tests/test_equalise_sanitize.py).
 * Per case: a picture of a random size (1 x 1 .. 200 x 90, now and then 8192 wide or 2000 high), grey or colour, noise, flat or two
 * values, with or without a mask (valid_step 1 or 8), a tile, a clip, an amount and a mode, now and then out of range, through the
 * model's tables and its apply, out of place and in place.  Every buffer is exactly as long as the interface says and comes from the
 * heap, so that one byte too far is a report.  Checked besides: every refusal has its code and text and writes nothing; the counts
 * add up to the counted pixels; every table of a tile that is not empty rises to 255; uncounted pixels stay; amount 0 changes nothing
 * in a grey picture; in place equals out of place.  Prints one JSON line.
 * Usage: fuzz_equalise <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "../../include/meteor_demod_amd_equalise.h"
#include "../../meteor_demod_amd/csrc/equalise_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

/* exactly `count` bytes, at a multiple of 4 as the interface asks (operator new gives 16) */
static std::unique_ptr<uint8_t[]> exact(size_t count) { return std::unique_ptr<uint8_t[]>(new uint8_t[count ? count : 1]); }

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 100;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	long refused = 0, accepted = 0, masked = 0, step8 = 0, colour = 0, wide = 0;
	unsigned long long tiles = 0, empty = 0, pixels = 0;
	for (long n = 0; n < cases; n++) {
		uint32_t width = 1 + static_cast<uint32_t>(rng() % (rng() % 4 == 0 ? 200 : 40)), height = 1 + static_cast<uint32_t>(rng() % (rng() % 4 == 0 ? 90 : 30));
		if (rng() % 25 == 0) { width = 8192; height = 1 + static_cast<uint32_t>(rng() % 20); wide++; }
		else if (rng() % 25 == 0) { height = 2000; width = 1 + static_cast<uint32_t>(rng() % 20); wide++; }
		uint32_t planes = rng() & 1 ? 3 : 1;
		mdemod_equalise_opts o;
		mdemod_equalise_default_opts(&o);
		o.tile = 8u * (2u + static_cast<uint32_t>(rng() % (rng() % 3 == 0 ? 63 : 6)));
		o.clip_percent = rng() % 3 == 0 ? 25600u : 100u + static_cast<uint32_t>(rng() % 1000);
		o.amount = static_cast<uint32_t>(rng() % 257);
		o.mode = static_cast<uint32_t>(rng() & 1);
		o.valid_step = rng() & 1 ? 8 : 1;
		bool fine = true;
		switch (rng() % 40) {
		case 0: width = rng() & 1 ? 0 : 8193; fine = false; break;
		case 1: height = rng() & 1 ? 0 : 16385; fine = false; break;
		case 2: planes = rng() & 1 ? 2 : 0; fine = false; break;
		case 3: o.tile = rng() & 1 ? 8 : 520; fine = false; break;
		case 4: o.tile += 4; fine = false; break;
		case 5: o.clip_percent = rng() & 1 ? 99 : 25601; fine = false; break;
		case 6: o.amount = 257 + static_cast<uint32_t>(rng() % 1000); fine = false; break;
		case 7: o.mode = 2 + static_cast<uint32_t>(rng() % 5); fine = planes == 1; break;
		case 8: o.valid_step = static_cast<uint32_t>(rng() % 3) * 2; fine = false; break;
		default: break;
		}
		const uint32_t w = width && width <= 8192 ? width : 8, h = height && height <= 16384 ? height : 8, pl = planes == 3 ? 3 : 1;
		const uint32_t step = o.valid_step == 8 ? 8 : 1;
		const size_t area = static_cast<size_t>(w) * h * pl, mask_bytes = static_cast<size_t>((h + step - 1) / step) * w;
		const bool with_mask = rng() % 3 != 0;
		auto pic = exact(area), valid = exact(mask_bytes), out = exact(area);
		const int kind = static_cast<int>(rng() % 3);
		for (size_t k = 0; k < area; k++) pic[k] = kind == 0 ? static_cast<uint8_t>(rng()) : kind == 1 ? 77 : (rng() % 8 == 0 ? 200 : 3);
		const int mkind = static_cast<int>(rng() % 3);
		for (size_t k = 0; k < mask_bytes; k++) valid[k] = mkind == 0 ? static_cast<uint8_t>(rng() & 1) : mkind == 1 ? (k % w < w / 2 ? 0 : 9) : 0;
		memset(out.get(), 0xA5, area);
		const uint8_t *mask = with_mask ? valid.get() : nullptr;

		const uint64_t need = mdemod_equalise_workspace(width, height, planes, &o);
		if ((need != 0) != fine) FAIL("case %ld: the workspace is %llu", n, (unsigned long long)need);
		const size_t room = need ? need : 260;
		auto work = exact(room);
		memset(work.get(), 0x5A, room);
		const int rc = mdemod_equalise_model_tables(pic.get(), mask, width, height, planes, &o, work.get(), room);
		if ((rc == MDEMOD_OK) != fine) { FAIL("case %ld: %u x %u x %u tile %u clip %u amount %u mode %u step %u came back %d", n, width, height, planes, o.tile, o.clip_percent, o.amount, o.mode, o.valid_step, rc); continue; }
		if (!fine) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: a refusal without its code or text", n);
			const int ra = mdemod_equalise_model_apply(pic.get(), mask, width, height, planes, &o, work.get(), out.get());
			if (ra != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: apply was not refused: %d", n, ra);
			bool clean = true;
			for (size_t k = 0; k < room; k++) clean = clean && work[k] == 0x5A;
			for (size_t k = 0; k < area; k++) clean = clean && out[k] == 0xA5;
			if (!clean) FAIL("case %ld: a refused call wrote", n);
			refused++;
			continue;
		}
		accepted++; masked += with_mask; step8 += with_mask && step == 8; colour += pl == 3; pixels += static_cast<unsigned long long>(w) * h;
		/* a workspace that is one byte short is refused, and nothing is written */
		if (need > 1) {
			auto small = exact(need - 1);
			memset(small.get(), 0x5A, need - 1);
			const int rs = mdemod_equalise_model_tables(pic.get(), mask, width, height, planes, &o, small.get(), need - 1);
			bool clean = true;
			for (size_t k = 0; k + 1 < need; k++) clean = clean && small[k] == 0x5A;
			if (rs != MDEMOD_ERR_PARAM || !clean) FAIL("case %ld: a workspace of %llu of %llu bytes came back %d", n, (unsigned long long)(need - 1), (unsigned long long)need, rs);
		}
		EqPlan p;
		if (eq_check("fuzz", width, height, planes, &o, &p) != MDEMOD_OK || eq_public_bytes(p) != need) { FAIL("case %ld: the plan", n); continue; }
		unsigned long long counted = 0, sum = 0;
		for (uint32_t y = 0; y < h; y++)
			for (uint32_t x = 0; x < w; x++) counted += !mask || mask[static_cast<size_t>(y / step) * w + x];
		const uint8_t *tab = work.get(), *cnt = work.get() + eq_tab_bytes(p);
		for (uint64_t t = 0; t < static_cast<uint64_t>(p.channels) * p.ny * p.nx; t++) {
			uint32_t c;
			memcpy(&c, cnt + 4 * t, 4);
			sum += c; tiles++; empty += c == 0;
			const uint8_t *row = tab + 256 * t;
			bool rises = true;
			for (int v = 1; v < 256; v++) rises = rises && row[v] >= row[v - 1];
			if (c ? (!rises || row[255] != 255) : (row[0] != 0 || row[255] != 0)) FAIL("case %ld: the table of tile %llu (n = %u)", n, (unsigned long long)t, c);
		}
		if (sum != counted * p.channels) FAIL("case %ld: the counts add up to %llu, %llu pixels are counted in %u channels", n, sum, counted, p.channels);
		if (mdemod_equalise_model_apply(pic.get(), mask, width, height, planes, &o, work.get(), out.get()) != MDEMOD_OK) { FAIL("case %ld: apply: %s", n, mdemod_last_error()); continue; }
		for (uint32_t y = 0; y < h; y++)
			for (uint32_t x = 0; x < w; x++) {
				const size_t at = (static_cast<size_t>(y) * w + x) * pl;
				const bool is_counted = !mask || mask[static_cast<size_t>(y / step) * w + x];
				if ((!is_counted || (o.amount == 0 && pl == 1)) && memcmp(out.get() + at, pic.get() + at, pl)) { FAIL("case %ld: pixel %u, %u changed", n, x, y); y = h; break; }
			}
		auto same = exact(area);
		memcpy(same.get(), pic.get(), area);
		if (mdemod_equalise_model_apply(same.get(), mask, width, height, planes, &o, work.get(), same.get()) != MDEMOD_OK || memcmp(same.get(), out.get(), area))
			FAIL("case %ld: in place differs from out of place", n);
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"bad\": %ld, \"refused\": %ld, \"accepted\": %ld, \"masked\": %ld, \"step8\": %ld, \"colour\": %ld, \"wide\": %ld, \"tiles\": %llu, "
	       "\"empty\": %llu, \"pixels\": %llu}\n", bad ? "false" : "true", cases, bad, refused, accepted, masked, step8, colour, wide, tiles, empty, pixels);
	return bad ? 1 : 0;
}
