/*
 * fuzz_interleave.cpp — the host side of the 80 k interleaved mode (csrc/interleave_host.cpp) under ASan + UBSan
 * (tests/test_interleave_sanitize.py): the tracker over made-up candidate lists (runs of (r, H), slips, noise windows, sometimes a
 * broken entry) and random options, and the model - the sync search on short streams, the gather over random segment tables
 * (sometimes broken ones) and branch delays up to the largest - with every buffer exactly as long as the interface says, so that a
 * byte read or written outside is a report.  Every accepted segment list is checked: segment 0 begins at symbol 0 and period 0,
 * first symbols ascend on window boundaries, periods do not descend, the sync word stands at the first symbol plus the phase, and
 * P is not below the last period; every refusal is MDEMOD_ERR_PARAM and leaves a text.  Prints one JSON line.
 * Usage: fuzz_interleave <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_interleave.h"
#include "../../meteor_demod_amd/csrc/interleave_host.h"

static long bad = 0;

static void
fail(long i, const char *what)
{
	fprintf(stderr, "case %ld: %s (%s)\n", i, what, mdemod_last_error());
	bad++;
}

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 3000;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	const uint64_t edges[] = { 0, 1, 3, 4, 5, 43, 44, 2562, 2563, 2564, 2565, 5122, 5123, 5124, 3 * 2560 + 17 };
	long tracked = 0, refused = 0, gathered = 0, gather_refused = 0, segments_seen = 0;
	for (long i = 0; i < cases; i++) {
		/* ---- the tracker ---- */
		const uint64_t m = (rng() & 3) == 0 ? edges[rng() % (sizeof(edges) / sizeof(edges[0]))] + 2560 * (rng() % 60) : rng() % (300 * 2560);
		const uint64_t nw = mdemod_il_windows(m);
		std::vector<mdemod_frames_candidate> cand(nw);
		uint32_t r = static_cast<uint32_t>(rng() % 40), H = static_cast<uint32_t>(rng() % 24);
		for (uint64_t w = 0; w < nw; w++) {
			const uint32_t dice = static_cast<uint32_t>(rng() % 16);
			if (dice == 0) r = static_cast<uint32_t>(rng() % 40);
			else if (dice == 1) r = (r + 39 + 2 * static_cast<uint32_t>(rng() % 2)) % 40;                  /* a slip of one symbol */
			else if (dice == 2) H = static_cast<uint32_t>(rng() % 24);
			uint32_t rr = dice >= 13 ? static_cast<uint32_t>(rng() % 40) : r;                             /* a noise window */
			const uint64_t positions = m - 3 - w * 2560 < 2560 ? m - 3 - w * 2560 : 2560;
			if (rr >= positions) rr = static_cast<uint32_t>(rng() % positions);
			cand[w].position = w * 2560 + rr;
			cand[w].hypothesis = dice >= 13 ? static_cast<uint32_t>(rng() % 24) : H;
			cand[w].score = static_cast<int32_t>(rng() % 131073) - 65536;
		}
		bool broken = false;
		if (nw && (rng() % 16) == 0) {
			broken = true;
			mdemod_frames_candidate &c = cand[rng() % nw];
			const uint32_t dice = static_cast<uint32_t>(rng() % 3);
			if (dice == 0) c.hypothesis = 24 + static_cast<uint32_t>(rng() % 1000);
			else if (dice == 1) c.position = c.position / 2560 * 2560 + 40 + rng() % 2520;
			else c.position += 2560 * (1 + rng() % 3);
		}
		mdemod_il_opts o;
		mdemod_il_default_opts(&o);
		if (rng() & 1) { o.min_run = static_cast<uint32_t>(rng() % 6); o.branch_delay = static_cast<uint32_t>(rng() % 4096); }
		if ((rng() % 32) == 0) o.min_run = 0xFFFFFFFFu;
		if ((rng() % 32) == 0) o.reserved[rng() & 1] = 1;
		const bool bad_opts = o.min_run == 0 || o.branch_delay == 0 || o.reserved[0] || o.reserved[1];
		const bool with_opts = (rng() & 7) != 0;
		const uint64_t cap = (rng() & 3) ? nw + 1 : rng() % (nw + 2);
		std::vector<mdemod_il_segment> seg(cap);                                                          /* (exactly: a write at [cap] is a report) */
		uint64_t n = 0xDEADBEEF, P = 0xDEADBEEF;
		const uint64_t claim = (rng() % 32) == 0 ? nw + 1 : nw;
		if (claim > nw) cand.resize(claim);
		const int rc = mdemod_il_track(with_opts ? &o : nullptr, cand.data(), claim, m, seg.data(), cap, &n, &P);
		if (rc != MDEMOD_OK) {
			refused++;
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || n != 0 || P != 0) fail(i, "a refusal that is not MDEMOD_ERR_PARAM with a text and zeroed counts");
			if (!broken && claim == nw && !(with_opts && bad_opts)) fail(i, "a good candidate list was refused");
		} else {
			tracked++;
			if (broken || claim != nw || (with_opts && bad_opts)) fail(i, "a broken candidate list or broken options were accepted");
			if (n > nw || (n == 0 && P != 0) || P > m) fail(i, "counts that do not fit the stream");
			for (uint64_t k = 0; k < n && k < cap; k++) {
				const mdemod_il_segment &s = seg[k];
				bool ok = s.phase < 40 && s.hypothesis < 24 && s.marker_symbol == s.first_symbol + s.phase && s.first_symbol % 2560 == 0 && s.marker_symbol + 4 <= m;
				if (k == 0) ok = ok && s.first_symbol == 0 && s.period == 0;
				else ok = ok && s.first_symbol > seg[k - 1].first_symbol && s.period >= seg[k - 1].period && (s.phase != seg[k - 1].phase || s.hypothesis != seg[k - 1].hypothesis);
				if (k + 1 == n) ok = ok && P == s.period + (m - s.marker_symbol) / 40;
				if (!ok) fail(i, "a segment that breaks the tracker's rules");
			}
			segments_seen += static_cast<long>(n);
		}

		/* ---- the model on a short stream: buffers exactly as long as the interface says ---- */
		if (i % 4) continue;
		const uint64_t ms = (rng() & 1) ? edges[rng() % (sizeof(edges) / sizeof(edges[0]))] : rng() % (4 * 2560);
		std::vector<int8_t> soft(2 * ms);
		for (int8_t &v : soft) v = static_cast<int8_t>(rng() & 0xFF);
		const uint64_t nws = mdemod_il_windows(ms);
		std::vector<mdemod_frames_candidate> cs(nws);
		if (mdemod_il_model_candidates(soft.data(), ms, cs.data()) != MDEMOD_OK) { fail(i, "the model's sync search refused a stream"); continue; }
		for (uint64_t w = 0; w < nws; w++)
			if (cs[w].position / 2560 != w || cs[w].position % 2560 >= 40 || cs[w].position + 4 > ms || cs[w].hypothesis >= 24 || cs[w].score > 65536 || cs[w].score < -65536)
				fail(i, "a model candidate outside its window");
		/* a segment table: what the tracker makes of the candidates (min_run 1), or a made-up one, sometimes broken */
		std::vector<mdemod_il_segment> table;
		uint64_t Ps = 0;
		bool broken_table = false;
		if (rng() & 1) {
			mdemod_il_opts t;
			mdemod_il_default_opts(&t);
			t.min_run = 1;
			table.resize(nws + 1);
			uint64_t ns = 0;
			if (mdemod_il_track(&t, cs.data(), nws, ms, table.data(), table.size(), &ns, &Ps) != MDEMOD_OK) { fail(i, "the tracker refused the model's candidates"); continue; }
			table.resize(ns);
		} else {
			const uint64_t ns = rng() % 6;
			uint64_t period = 0;
			for (uint64_t k = 0; k < ns; k++) {
				mdemod_il_segment s = { 0, ms ? rng() % (ms + 1) : 0, period, 0, static_cast<uint32_t>(rng() % 24) };
				table.push_back(s);
				period += rng() % 40;
			}
			Ps = ns ? rng() % (ms + 1) : 0;
			if (ns && (rng() % 4) == 0) {
				broken_table = true;
				const uint32_t dice = static_cast<uint32_t>(rng() % 4);
				mdemod_il_segment &s = table[rng() % ns];
				if (dice == 0) s.hypothesis = 24 + static_cast<uint32_t>(rng() % 100);
				else if (dice == 1) s.marker_symbol = ms + 1 + rng() % 1000;
				else if (dice == 2) table[0].period = 1 + rng() % 5;
				else Ps = ms + 1 + rng() % 1000;
			}
		}
		mdemod_il_opts g;
		mdemod_il_default_opts(&g);
		const uint32_t dice = static_cast<uint32_t>(rng() % 8);
		g.branch_delay = dice == 0 ? 0xFFFFFFFFu : dice == 1 ? 2048u : 1u + static_cast<uint32_t>(rng() % 12);
		std::vector<int8_t> out(72 * Ps);
		const int grc = mdemod_il_model_deinterleave(&g, soft.data(), ms, table.data(), table.size(), Ps, out.data());
		if (grc != MDEMOD_OK) {
			gather_refused++;
			if (grc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || !broken_table) fail(i, "the gather refused a good table, or without MDEMOD_ERR_PARAM and a text");
		} else {
			gathered++;
			if (broken_table) fail(i, "a broken segment table was accepted");
		}
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"tracked\": %ld, \"refused\": %ld, \"gathered\": %ld, \"gather_refused\": %ld, \"segments\": %ld, \"bad\": %ld}\n",
	       bad ? "false" : "true", cases, tracked, refused, gathered, gather_refused, segments_seen, bad);
	return bad ? 1 : 0;
}
