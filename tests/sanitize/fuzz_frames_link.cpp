/*
 * fuzz_frames_link.cpp — the link variant of the frame layer (csrc/frames_host.cpp, csrc/frames_link_host.cpp) under ASan + UBSan
 * (tests/test_frames_link_host.py): the tracker's link entry and the link model over random modes (differential, skew, sometimes a
 * broken struct), candidate lists with H = h + 8 s, options and short soft streams.  Every accepted frame list is checked: no more
 * frames than the stream has room for, every frame complete, positions ascending, no two frames overlap, a hypothesis the mode
 * allows, a frame without the flywheel flag stands on a candidate; every refusal is MDEMOD_ERR_PARAM and leaves a text.  The model
 * is run on short streams (random bytes over the full int8 range, lengths around the edges, the reads at index m among them) and
 * its candidates are checked against their windows.  Prints one JSON line.
 * Usage: fuzz_frames_link <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_frames_link.h"
#include "../../meteor_demod_amd/csrc/frames_host.h"

static long bad = 0;

static bool
allowed(uint32_t H, const mdemod_frames_link &l)
{
	return H < (l.skew ? 24u : 8u) && !(l.differential && (H & 2u));
}

static void
check_list(long i, const std::vector<mdemod_frame_info> &fr, uint64_t n, uint64_t cap, uint64_t m, const std::vector<mdemod_frames_candidate> *cand, const mdemod_frames_link &l)
{
	if (n > m / 8192) { fprintf(stderr, "case %ld: %llu frames in %llu symbols\n", i, (unsigned long long)n, (unsigned long long)m); bad++; }
	const uint64_t shown = n < cap ? n : cap;
	for (uint64_t k = 0; k < shown; k++) {
		const mdemod_frame_info &f = fr[k];
		bool ok = f.position + 8192 <= m && allowed(f.hypothesis, l) && (k == 0 || f.position >= fr[k - 1].position + 8192) && (f.flags & ~MDEMOD_FRAME_FLYWHEEL) == 0;
		if (ok && cand && !(f.flags & MDEMOD_FRAME_FLYWHEEL)) {
			const mdemod_frames_candidate &c = (*cand)[f.position / 8192];
			ok = c.position == f.position && c.hypothesis == f.hypothesis && c.score == f.score;
		}
		if (!ok) { fprintf(stderr, "case %ld: frame %llu at %llu (h %u, flags %u) in %llu symbols\n", i, (unsigned long long)k, (unsigned long long)f.position, f.hypothesis, f.flags, (unsigned long long)m); bad++; }
	}
}

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 3000;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	const uint64_t edges[] = { 0, 1, 31, 32, 33, 34, 35, 8191, 8192, 8193, 8223, 8224, 8225, 8226, 16384, 16416, 3 * 8192 + 5000 };
	long tracked = 0, refused = 0, decoded = 0, frames_seen = 0;
	for (long i = 0; i < cases; i++) {
		/* ---- the tracker on a made-up candidate list: a few runs of (r, h), slips, noise windows, sometimes a broken entry ---- */
		const uint64_t m = (rng() & 3) == 0 ? edges[rng() % (sizeof(edges) / sizeof(edges[0]))] + 8192 * (rng() % 40) : rng() % (200 * 8192);
		mdemod_frames_link link = { static_cast<uint32_t>(rng() & 1), static_cast<uint32_t>(rng() & 1), { 0, 0 } };
		const uint32_t span = 32 + link.skew, hyps = link.skew ? 24 : 8;
		auto pick = [&]() { uint32_t H; do H = static_cast<uint32_t>(rng() % hyps); while (!allowed(H, link)); return H; };
		const uint64_t nw = mdemod_frames_link_windows(&link, m);
		std::vector<mdemod_frames_candidate> cand(nw);
		uint32_t r = static_cast<uint32_t>(rng() % 8192), h = pick();
		for (uint64_t w = 0; w < nw; w++) {
			const uint32_t dice = static_cast<uint32_t>(rng() % 16);
			if (dice == 0) r = static_cast<uint32_t>(rng() % 8192);
			else if (dice == 1) r = (r + 8191 + 2 * static_cast<uint32_t>(rng() % 2)) % 8192;           /* a slip of one symbol */
			else if (dice == 2) h = pick();
			uint32_t rr = dice >= 12 ? static_cast<uint32_t>(rng() % 8192) : r;                         /* a noise window */
			const uint64_t positions = m - span - w * 8192 < 8192 ? m - span - w * 8192 : 8192;
			if (rr >= positions) rr = static_cast<uint32_t>(rng() % positions);
			cand[w].position = w * 8192 + rr;
			cand[w].hypothesis = dice >= 12 ? pick() : h;
			cand[w].score = static_cast<int32_t>(rng() % 13313) - 6656;
		}
		bool broken = false;
		if (nw && (rng() % 16) == 0) {
			broken = true;
			mdemod_frames_candidate &c = cand[rng() % nw];
			const uint32_t dice = static_cast<uint32_t>(rng() % 3);
			if (dice == 0) c.hypothesis = hyps + static_cast<uint32_t>(rng() % 1000);
			else if (dice == 1 && link.differential) c.hypothesis |= 2u;
			else c.position += 8192 * (1 + rng() % 3);
		}
		mdemod_frames_opts o;
		mdemod_frames_default_opts(&o);
		if (rng() & 1) { o.min_run = static_cast<uint32_t>(rng() % 6); o.flywheel = static_cast<uint32_t>(rng() % 8); }
		if ((rng() % 32) == 0) o.flywheel = 0xFFFFFFFFu;
		if ((rng() % 32) == 0) o.min_run = 0xFFFFFFFFu;
		if ((rng() % 32) == 0) o.piece_symbols = rng() % 100000;
		const uint64_t cap = (rng() & 3) ? m / 8192 + 1 : rng() % (m / 8192 + 2);
		std::vector<mdemod_frame_info> fr(cap + 1);
		uint64_t n = 0xDEADBEEF;
		const uint64_t claim = (rng() % 32) == 0 ? nw + 1 : nw;
		if (claim > nw) cand.resize(claim);
		mdemod_frames_link sent = link;
		bool broken_link = false;
		if ((rng() % 32) == 0) { broken_link = true; if (rng() & 1) sent.skew = 2 + static_cast<uint32_t>(rng() % 5); else sent.reserved[rng() & 1] = 1; }
		const int rc = mdemod_frames_link_track(&sent, (rng() & 7) ? &o : nullptr, cand.data(), claim, m, fr.data(), cap, &n);
		if (rc != MDEMOD_OK) {
			refused++;
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || n != 0) { fprintf(stderr, "case %ld: track rc %d, n %llu, text '%s'\n", i, rc, (unsigned long long)n, mdemod_last_error()); bad++; }
		} else {
			tracked++;
			if (broken || broken_link || claim != nw) { fprintf(stderr, "case %ld: a broken candidate list was accepted\n", i); bad++; }
			else check_list(i, fr, n, cap, m, &cand, link);
			frames_seen += static_cast<long>(n);
		}

		/* ---- the model on a short stream: sometimes noise, sometimes an encoded run of frames in it ---- */
		if (i % 8) continue;
		const uint64_t ms = (rng() & 1) ? edges[rng() % (sizeof(edges) / sizeof(edges[0]))] : rng() % (6 * 8192);
		std::vector<int8_t> soft(2 * ms);                                                              /* (exactly: a read at index m is a report) */
		for (int8_t &v : soft) v = static_cast<int8_t>(rng() & 0xFF);
		if ((rng() & 1) && ms > 8192) {
			std::vector<uint8_t> bytes(ms / 8 + 1);
			for (uint8_t &b : bytes) b = static_cast<uint8_t>(rng() & 0xFF);
			const uint64_t lead = rng() % 1024;                                                          /* bytes before the first marker */
			for (uint64_t at = lead; at + 4 <= bytes.size(); at += 1024) { bytes[at] = 0x1A; bytes[at + 1] = 0xCF; bytes[at + 2] = 0xFC; bytes[at + 3] = 0x1D; }
			if (link.differential) {                                                                      /* the sender's NRZ-M */
				uint32_t d = 0;
				for (uint8_t &b : bytes) { uint8_t out = 0; for (int k = 7; k >= 0; k--) { d ^= (b >> k) & 1u; out |= static_cast<uint8_t>(d << k); } b = out; }
			}
			std::vector<int8_t> sym(16 * bytes.size());
			(void)mdemod_frames_model_encode(bytes.data(), bytes.size(), 0, sym.data());
			const int amp = 1 + static_cast<int>(rng() % 127);
			for (uint64_t k = 0; k < 2 * ms; k++) {
				const int v = sym[k] * amp + static_cast<int>(rng() % 9) - 4;
				soft[k] = static_cast<int8_t>(v > 127 ? 127 : (v < -128 ? -128 : v));
			}
		}
		const uint64_t nws = mdemod_frames_link_windows(&link, ms);
		std::vector<mdemod_frames_candidate> cs(nws + 1);
		if (mdemod_frames_model_link_candidates(&link, soft.data(), ms, cs.data()) != MDEMOD_OK) { fprintf(stderr, "case %ld: model candidates refused %llu symbols\n", i, (unsigned long long)ms); bad++; continue; }
		for (uint64_t w = 0; w < nws; w++)
			if (cs[w].position / 8192 != w || cs[w].position + span >= ms || !allowed(cs[w].hypothesis, link) || cs[w].score > 6656 || cs[w].score < 0) {
				fprintf(stderr, "case %ld: model candidate %llu at %llu score %d\n", i, (unsigned long long)w, (unsigned long long)cs[w].position, cs[w].score); bad++;
			}
		const uint64_t caps = ms / 8192 + 1;
		std::vector<mdemod_frame_info> fs(caps);
		std::vector<uint8_t> cadu(caps * 1024);
		uint64_t ns = 0;
		mdemod_frames_opts om;
		mdemod_frames_default_opts(&om);
		om.min_run = 1 + static_cast<uint32_t>(rng() % 3);
		if (mdemod_frames_model_link_decode(&link, &om, soft.data(), ms, cadu.data(), fs.data(), caps, &ns) != MDEMOD_OK) { fprintf(stderr, "case %ld: model decode refused: %s\n", i, mdemod_last_error()); bad++; continue; }
		decoded++;
		check_list(i, fs, ns, caps, ms, nullptr, link);
		for (uint64_t k = 0; k < ns && k < caps; k++)
			if (fs[k].channel_errors > MDEMOD_FRAME_DECISIONS) { fprintf(stderr, "case %ld: %u channel errors\n", i, fs[k].channel_errors); bad++; }
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"tracked\": %ld, \"refused\": %ld, \"decoded\": %ld, \"frames\": %ld, \"bad\": %ld}\n", bad ? "false" : "true", cases,
	       tracked, refused, decoded, frames_seen, bad);
	return bad ? 1 : 0;
}
