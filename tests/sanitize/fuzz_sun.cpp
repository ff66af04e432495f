/*
 * fuzz_sun.cpp — the host side of the sun layer (csrc/sun_host.cpp over csrc/map_host.cpp) under ASan + UBSan
 * (tests/test_sun_sanitize.py).  Per case: a picture of 1 .. 24 strip rows (now and then 300), a slot mask (now and then out of
 * range) and a gain table - random words below 2^22 with missing nodes, or the nodes of a pass of the element set given, at a random
 * time, date, scan angle (up to 130 degrees: nodes off the Earth), limit and reference (now and then out of range) - through the
 * model's apply, out of place and in place, and through the host entry's model with random APIDs.  Every buffer is exactly as long as
 * the interface says and comes from the heap, so that one byte too far is a report.  Checked besides: every refusal has its code and
 * text and writes nothing; a cell with a missing corner is copied, zeroes stay zero, a corrected byte lies between what the smallest and the
 * largest corner alone would give; the counts are at least those of the pixels that the smallest corner alone holds at 255, and 0 for a
 * slot that is not selected; slots that are not selected are not touched; in
 * place equals out of place; the host entry corrects exactly the slots of APID 64 .. 66.  Prints one JSON line.
 * Usage: fuzz_sun <cases> <seed> <tle file>
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/meteor_demod_amd_sun.h"
#include "../../meteor_demod_amd/csrc/sun_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

/* exactly `count` bytes, at a multiple of 4 as the interface asks (operator new gives 16) */
static std::unique_ptr<uint8_t[]> exact(size_t count) { return std::unique_ptr<uint8_t[]>(new uint8_t[count ? count : 1]); }

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 100;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	if (argc < 4) { fprintf(stderr, "usage: fuzz_sun <cases> <seed> <tle file>\n"); return 2; }
	std::string text;
	if (FILE *f = fopen(argv[3], "rb")) {
		char buf[4096];
		size_t got;
		while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
		fclose(f);
	}
	mdemod_map_tle tle;
	if (mdemod_map_parse_tle(text.c_str(), 0, &tle) != MDEMOD_OK) { fprintf(stderr, "no element set in %s: %s\n", argv[3], mdemod_last_error()); return 2; }

	long refused = 0, accepted = 0, missing_tables = 0, in_place = 0, node_tables = 0, nodes_off_earth = 0, hosts = 0, masks[8] = { 0 };
	unsigned long long pixels = 0, saturated = 0;
	for (long n = 0; n < cases; n++) {
		uint32_t rows = 1 + static_cast<uint32_t>(rng() % 24);
		if (rng() % 30 == 0) rows = 300;
		uint32_t mask = 1 + static_cast<uint32_t>(rng() % 7);
		mdemod_sun_opts so;
		mdemod_map_opts mo;
		mdemod_sun_default_opts(&so);
		mdemod_map_default_opts(&mo);
		so.limit_deg = 60.0 + static_cast<double>(rng() % 2901) / 100.0;
		so.ref_deg = static_cast<double>(rng() % 8001) / 100.0;
		mo.scan_deg = rng() % 3 == 0 ? 124.0 + static_cast<double>(rng() % 61) / 10.0 : 60.0 + static_cast<double>(rng() % 600) / 10.0;
		mo.side = rng() & 1 ? 1 : -1;
		mo.date = tle.epoch_day + static_cast<int32_t>(rng() % 400) - 200;
		bool fine_nodes = true, fine_apply = true;
		switch (rng() % 24) {
		case 0: so.limit_deg = rng() & 1 ? 59.99 : 89.01; fine_nodes = false; break;
		case 1: so.limit_deg = rng() & 1 ? NAN : INFINITY; fine_nodes = false; break;
		case 2: so.ref_deg = rng() & 1 ? -0.01 : 80.01; fine_nodes = false; break;
		case 3: mo.scan_deg = rng() & 1 ? 0.5 : 130.5; fine_nodes = false; break;
		case 4: rows = rng() & 1 ? 0 : MDEMOD_SUN_MAX_ROWS + 1 + static_cast<uint32_t>(rng() % 100); fine_nodes = fine_apply = false; break;
		case 5: mask = rng() & 1 ? 0 : 8 + static_cast<uint32_t>(rng() % 1000); fine_apply = false; break;
		default: break;
		}
		const uint32_t r = rows >= 1 && rows <= MDEMOD_SUN_MAX_ROWS ? rows : 2;      /* what the buffers are sized for */
		const size_t area = static_cast<size_t>(r) * SUN_ROW_BYTES, words = (static_cast<size_t>(r) + 1) * MDEMOD_SUN_NODE_COLS;
		auto table = exact(words * 4);
		uint32_t *gain = reinterpret_cast<uint32_t *>(table.get());

		/* the packets of a pass that loses nothing: one image packet per row, slot and cell would do; one per row is enough for the fit */
		std::vector<mdemod_placement> place(r);
		std::vector<mdemod_strip_info> sinfo(r);
		const double s0 = static_cast<double>(rng() % 86400), period = 1.230769;
		for (uint32_t k = 0; k < r; k++) {
			const long long us = llround(fmod(s0 + period * k, 86400.0) * 1e6);
			place[k] = mdemod_placement{ static_cast<int32_t>(k % 3), k, k % 14, 0 };
			sinfo[k] = mdemod_strip_info{ 14, 60, static_cast<uint8_t>(14 * (k % 14)), 0, 7, static_cast<uint16_t>(us % 1000), static_cast<uint32_t>(us / 1000), 900 };
		}

		/* ---- the table: a pass's nodes, or random words ---- */
		const bool from_pass = rng() % 2 == 0 || !fine_nodes;
		bool has_missing = false;
		if (from_pass) {
			mdemod_map_timing tm;
			if (mdemod_map_fit_time(place.data(), sinfo.data(), r, &mo, &tm) != MDEMOD_OK) {
				if (mo.scan_deg >= 1.0 && mo.scan_deg <= 130.0) FAIL("case %ld: the line times: %s", n, mdemod_last_error());
				tm.row_period = period; tm.s0 = s0; tm.date = mo.date; tm.rows_fit = r; tm.placed = r; tm.lines = 8 * r;
			}
			memset(gain, 0x5A, words * 4);
			mdemod_sun_summary ss;
			memset(&ss, 0x77, sizeof ss);
			mdemod_sun_orbit orbit;
			mdemod_sun_timing timing;
			mdemod_sun_pass_opts po;
			const int rc = mdemod_sun_nodes(sun_twin(&tle, orbit), sun_twin(&tm, timing), sun_twin(&mo, po), &so, rows, gain, &ss);
			if ((rc == MDEMOD_OK) != fine_nodes) { FAIL("case %ld: nodes of %u rows, limit %g, ref %g, scan %g came back %d", n, rows, so.limit_deg, so.ref_deg, mo.scan_deg, rc); continue; }
			if (!fine_nodes) {
				bool clean = rc == MDEMOD_ERR_PARAM && *mdemod_last_error();
				for (size_t k = 0; k < words; k++) clean = clean && gain[k] == 0x5A5A5A5Au;
				const uint8_t *sb = reinterpret_cast<const uint8_t *>(&ss);
				for (size_t k = 0; k < sizeof ss; k++) clean = clean && sb[k] == 0x77;
				if (!clean) FAIL("case %ld: a refused mdemod_sun_nodes wrote, or has no text", n);
				refused++;
				if (!fine_apply) continue;
				for (size_t k = 0; k < words; k++) gain[k] = 65536;
			} else {
				node_tables++;
				uint32_t miss = 0, at = 0;
				const uint32_t top = static_cast<uint32_t>(floor(65536.0 * cos(so.ref_deg * M_PI / 180.0) / cos(so.limit_deg * M_PI / 180.0) + 0.5));
				for (size_t k = 0; k < words; k++) {
					miss += gain[k] == MDEMOD_SUN_NO_NODE;
					at += gain[k] == top;
					if (gain[k] != MDEMOD_SUN_NO_NODE && (gain[k] > top || gain[k] >= (1u << 22) || gain[k] < 11380)) { FAIL("case %ld: node %zu is %u (the limit's gain is %u)", n, k, gain[k], top); break; }
				}
				if (miss != ss.missing || ss.nodes != words || ss.at_limit > words - miss || at < ss.at_limit || ss.date != mo.date || ss.slot_mask || ss.saturated[0])
					FAIL("case %ld: the summary: %u of %u missing (counted %u), %u at the limit (counted %u)", n, ss.missing, ss.nodes, miss, ss.at_limit, at);
				if (miss < words && !(ss.zenith_min >= 0.0 && ss.zenith_min <= ss.zenith_max && ss.zenith_max <= 180.0)) FAIL("case %ld: zenith %g .. %g", n, ss.zenith_min, ss.zenith_max);
				if (miss && mo.scan_deg < 120.0) FAIL("case %ld: %u nodes off the Earth at a scan angle of %g", n, miss, mo.scan_deg);
				nodes_off_earth += miss > 0;
				has_missing = miss > 0;
			}
		} else {
			const int kind = static_cast<int>(rng() % 3);
			for (size_t k = 0; k < words; k++) {
				gain[k] = kind == 0 ? static_cast<uint32_t>(rng() % (1u << 22)) : kind == 1 ? 65536u + static_cast<uint32_t>(rng() % 400000) : (1u << 22) - 1u;
				if (rng() % 9 == 0) { gain[k] = MDEMOD_SUN_NO_NODE; has_missing = true; }
			}
		}

		/* ---- the model's apply ---- */
		std::unique_ptr<uint8_t[]> in[3], out[3];
		const uint8_t *image[3];
		uint8_t *outp[3];
		for (int k = 0; k < 3; k++) {
			in[k] = exact(area); out[k] = exact(area);
			const int kind = static_cast<int>(rng() % 3);
			for (size_t i = 0; i < area; i++) in[k][i] = kind == 0 ? static_cast<uint8_t>(rng()) : kind == 1 ? (rng() % 4 == 0 ? 255 : 0) : static_cast<uint8_t>(i % 251);
			memset(out[k].get(), 0xA5, area);
			image[k] = in[k].get(); outp[k] = out[k].get();
		}
		/* what is not selected is not looked at: now and then it is not there */
		const uint32_t m7 = mask & 7u;
		if (fine_apply && rng() % 3 == 0) for (int k = 0; k < 3; k++) if (!(m7 >> k & 1u)) { image[k] = nullptr; outp[k] = rng() & 1 ? nullptr : reinterpret_cast<uint8_t *>(1); }
		uint64_t sat[3] = { 99, 99, 99 };
		const int rc = mdemod_sun_model_apply(image, outp, mask, rows, gain, sat);
		if ((rc == MDEMOD_OK) != fine_apply) { FAIL("case %ld: apply of %u rows under mask %u came back %d", n, rows, mask, rc); continue; }
		if (!fine_apply) {
			bool clean = rc == MDEMOD_ERR_PARAM && *mdemod_last_error() && sat[0] == 99 && sat[1] == 99 && sat[2] == 99;
			for (int k = 0; k < 3; k++) for (size_t i = 0; i < area; i++) clean = clean && out[k][i] == 0xA5;
			if (!clean) FAIL("case %ld: a refused mdemod_sun_model_apply wrote, or has no text", n);
			refused++;
			continue;
		}
		accepted++; masks[mask]++; missing_tables += has_missing; pixels += static_cast<unsigned long long>(area);
		for (int k = 0; k < 3; k++) {
			if (!(mask >> k & 1u)) {
				bool clean = sat[k] == 0;
				for (size_t i = 0; i < area; i++) clean = clean && out[k][i] == 0xA5;
				if (!clean) FAIL("case %ld: slot %d is not selected and was touched", n, k);
				continue;
			}
			uint64_t held = 0;
			for (uint32_t y = 0; y < 8 * r && bad < 20; y++)
				for (uint32_t x = 0; x < SUN_WIDTH; x++) {
					const uint32_t *g0 = gain + static_cast<size_t>(y >> 3) * MDEMOD_SUN_NODE_COLS + (x >> 4), *g1 = g0 + MDEMOD_SUN_NODE_COLS;
					const bool miss = g0[0] == MDEMOD_SUN_NO_NODE || g0[1] == MDEMOD_SUN_NO_NODE || g1[0] == MDEMOD_SUN_NO_NODE || g1[1] == MDEMOD_SUN_NO_NODE;
					const uint32_t lo = std::min(std::min(g0[0], g0[1]), std::min(g1[0], g1[1])), hi = std::max(std::max(g0[0], g0[1]), std::max(g1[0], g1[1]));
					const size_t at = static_cast<size_t>(y) * SUN_WIDTH + x;
					const uint32_t v = in[k][at], o = out[k][at];
					if (miss) { if (o != v) { FAIL("case %ld: pixel %u, %u of slot %d under a missing node changed", n, x, y, k); y = 8 * r; break; } continue; }
					/* between what the smallest and the largest corner alone would give, and held at 255 exactly when the sum passes it */
					const uint32_t a = std::min(255u, (v * lo + 32768u) >> 16), b = std::min(255u, (v * hi + 32768u) >> 16);
					if (o < a || o > b || (!v && o)) { FAIL("case %ld: pixel %u, %u of slot %d: %u became %u (corners %u .. %u)", n, x, y, k, v, o, lo, hi); y = 8 * r; break; }
					held += ((v * lo + 32768u) >> 16) > 255u;
				}
			if (sat[k] < held) FAIL("case %ld: slot %d: %llu saturated, %llu at least", n, k, (unsigned long long)sat[k], (unsigned long long)held);
			saturated += sat[k];
		}
		/* in place equals out of place */
		if (rng() % 3 != 0) {
			in_place++;
			std::unique_ptr<uint8_t[]> same[3];
			const uint8_t *si[3] = { nullptr, nullptr, nullptr };
			uint8_t *sp[3] = { nullptr, nullptr, nullptr };
			for (int k = 0; k < 3; k++) {
				if (!(mask >> k & 1u)) continue;
				same[k] = exact(area);
				memcpy(same[k].get(), in[k].get(), area);
				si[k] = sp[k] = same[k].get();
			}
			uint64_t sat2[3];
			if (mdemod_sun_model_apply(si, sp, mask, rows, gain, sat2) != MDEMOD_OK) FAIL("case %ld: in place: %s", n, mdemod_last_error());
			else for (int k = 0; k < 3; k++)
				if ((mask >> k & 1u) && (memcmp(same[k].get(), out[k].get(), area) || sat2[k] != sat[k])) FAIL("case %ld: slot %d in place differs from out of place", n, k);
		}

		/* ---- the host entry's model: the slots of APID 64 .. 66, and no other ---- */
		if (fine_nodes && rng() % 2 == 0) {
			hosts++;
			uint32_t apids[3];
			for (int k = 0; k < 3; k++) apids[k] = 62 + static_cast<uint32_t>(rng() % 8);
			uint8_t *pic[3];
			std::unique_ptr<uint8_t[]> copy[3];
			for (int k = 0; k < 3; k++) { copy[k] = exact(area); memcpy(copy[k].get(), in[k].get(), area); pic[k] = copy[k].get(); }
			mdemod_sun_summary ss;
			mdemod_sun_orbit orbit;
			mdemod_sun_pass_opts po;
			const int rh = mdemod_sun_model_host(&so, sun_twin(&mo, po), sun_twin(&tle, orbit), pic, apids, rows, place.data(), sinfo.data(), r, &ss);
			if (rh != MDEMOD_OK) { FAIL("case %ld: the host entry: %s", n, mdemod_last_error()); continue; }
			for (int k = 0; k < 3; k++) {
				const bool reflective = apids[k] >= 64 && apids[k] <= 66;
				if (((ss.slot_mask >> k & 1u) != 0) != reflective) FAIL("case %ld: APID %u in slot %d, mask %u", n, apids[k], k, ss.slot_mask);
				if (!reflective && (memcmp(copy[k].get(), in[k].get(), area) || ss.saturated[k])) FAIL("case %ld: slot %d (APID %u) was touched", n, k, apids[k]);
			}
		}
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"bad\": %ld, \"refused\": %ld, \"accepted\": %ld, \"missing_tables\": %ld, \"in_place\": %ld, \"node_tables\": %ld, "
	       "\"nodes_off_earth\": %ld, \"hosts\": %ld, \"masks\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld], \"pixels\": %llu, \"saturated\": %llu}\n", bad ? "false" : "true", cases, bad,
	       refused, accepted, missing_tables, in_place, node_tables, nodes_off_earth, hosts, masks[1], masks[2], masks[3], masks[4], masks[5], masks[6], masks[7], pixels, saturated);
	return bad ? 1 : 0;
}
