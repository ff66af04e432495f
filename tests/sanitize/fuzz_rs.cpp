/*
 * fuzz_rs.cpp — the host model of the transfer-frame layer (csrc/rs_host.cpp) under ASan + UBSan (tests/test_rs_host.py): random
 * options (some out of range: refused with MDEMOD_ERR_PARAM and a text, nothing written), 0 .. 9 frames, 0 .. 40 byte errors in
 * every codeword.  The decoding rule is asserted for every word: up to 16 errors come back as the bytes that were encoded, with the
 * count; more than 16 read 255 and leave the word as received (a codeword within 16 of such a word has probability about 1 / 16!:
 * one would be counted as a false correction, and the run fails).  Every encoded word is checked against syndromes computed here,
 * with a product of this file's own.  Prints one JSON line.
 * Usage: fuzz_rs <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_rs.h"
#include "../../meteor_demod_amd/csrc/rs_host.h"

static long bad = 0;

static uint8_t
product(uint8_t a, uint8_t b)
{
	unsigned acc = 0, x = a;
	for (int i = 0; i < 8; i++) {
		if (b >> i & 1) acc ^= x;
		x <<= 1;
		if (x & 0x100) x ^= 0x187;
	}
	return static_cast<uint8_t>(acc);
}

static uint8_t
power(uint8_t a, unsigned e)
{
	uint8_t r = 1;
	while (e--) r = product(r, a);
	return r;
}

/* the four words of a frame body as the decoder sees them have 32 zero syndromes */
static bool
is_codeword(const uint8_t *body, int c, const uint8_t *pn, const uint8_t *Tinv, const mdemod_rs_opts &o, const uint8_t roots[32])
{
	for (int k = 0; k < 32; k++) {
		uint8_t acc = 0;
		for (int i = 0; i < 255; i++) {
			uint8_t v = body[4 * i + c];
			if (o.derandomise) v ^= pn[(4 * i + c) % 255];
			if (o.dual_basis) v = Tinv[v];
			acc = product(acc, roots[k]) ^ v;
		}
		if (acc) return false;
	}
	return true;
}

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 400;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	uint8_t pn[255], T[256], Tinv[256], roots[32];
	mdemod_rs_model_pn(pn);
	mdemod_rs_model_dual(T, Tinv);
	for (int k = 0; k < 32; k++) roots[k] = power(2, (11u * (112u + k)) % 255u);
	long refused = 0, words = 0, clean = 0, corrected = 0, failed = 0, false_corrections = 0;
	for (long i = 0; i < cases; i++) {
		mdemod_rs_opts o;
		mdemod_rs_default_opts(&o);
		o.derandomise = static_cast<uint32_t>(rng() & 1);
		o.dual_basis = static_cast<uint32_t>(rng() & 1);
		if ((rng() & 3) == 0) o.piece_frames = rng() % 100;
		bool broken = false;
		if ((rng() % 12) == 0) {
			broken = true;
			switch (rng() % 3) {
			case 0: o.derandomise = 2 + static_cast<uint32_t>(rng() % 1000); break;
			case 1: o.dual_basis = 2 + static_cast<uint32_t>(rng() % 1000); break;
			default: o.piece_frames = (1ull << 20) + 1 + rng() % 1000; break;
			}
		}
		const uint64_t n = rng() % 10;
		std::vector<uint8_t> sent(n * 892 + 1), cadu(n * 1024 + 1), received(n * 892 + 1), out(n * 892 + 1, 0xEE);
		std::vector<mdemod_rs_info> info(n + 1);
		std::vector<int> errors(n * 4 + 1);
		memset(info.data(), 0xEE, info.size() * sizeof(mdemod_rs_info));
		for (uint8_t &v : sent) v = static_cast<uint8_t>(rng());
		if (broken) {
			uint8_t one[1024];
			const int rc = n ? mdemod_rs_model_decode(&o, cadu.data(), n, out.data(), info.data()) : mdemod_rs_model_encode(&o, sent.data(), one);
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) { fprintf(stderr, "case %ld: options out of range gave rc %d, text '%s'\n", i, rc, mdemod_last_error()); bad++; }
			for (uint64_t k = 0; k < n * 892; k++) if (out[k] != 0xEE) { fprintf(stderr, "case %ld: a refused call wrote\n", i); bad++; break; }
			refused++;
			continue;
		}
		mdemod_rs_opts defaults;
		mdemod_rs_default_opts(&defaults);
		const bool by_default = o.derandomise == defaults.derandomise && o.dual_basis == defaults.dual_basis && (rng() & 1);
		for (uint64_t f = 0; f < n; f++) {
			uint8_t *row = cadu.data() + f * 1024;
			if (mdemod_rs_model_encode(by_default ? nullptr : &o, sent.data() + f * 892, row) != MDEMOD_OK) { fprintf(stderr, "case %ld: encode refused: %s\n", i, mdemod_last_error()); bad++; }
			if (row[0] != 0x1A || row[1] != 0xCF || row[2] != 0xFC || row[3] != 0x1D) { fprintf(stderr, "case %ld: no marker\n", i); bad++; }
			for (int c = 0; c < 4; c++) {
				if (!is_codeword(row + 4, c, pn, Tinv, o, roots)) { fprintf(stderr, "case %ld: frame %llu codeword %d has a syndrome\n", i, (unsigned long long)f, c); bad++; }
				const int e = static_cast<int>(rng() % 41);
				errors[f * 4 + c] = e;
				bool hit[255] = { false };
				for (int k = 0; k < e;) {
					const int p = static_cast<int>(rng() % 255);
					if (hit[p]) continue;
					hit[p] = true;
					row[4 + 4 * p + c] ^= static_cast<uint8_t>(1 + rng() % 255);
					k++;
				}
			}
			for (int k = 0; k < 892; k++) received[f * 892 + k] = static_cast<uint8_t>(row[4 + k] ^ (o.derandomise ? pn[k % 255] : 0));
		}
		const int rc = mdemod_rs_model_decode(by_default ? nullptr : &o, cadu.data(), n, out.data(), info.data());
		if (rc != MDEMOD_OK) { fprintf(stderr, "case %ld: decode refused: %s\n", i, mdemod_last_error()); bad++; continue; }
		if (out[n * 892] != 0xEE || info[n].flags != 0xEEEEEEEEu) { fprintf(stderr, "case %ld: written past the end\n", i); bad++; }
		for (uint64_t f = 0; f < n; f++) {
			uint32_t want_flags = 0;
			for (int c = 0; c < 4; c++) {
				const int e = errors[f * 4 + c], got = info[f].corrected[c];
				words++;
				bool as_sent = true, as_received = true;
				for (int k = c; k < 892; k += 4) {
					as_sent = as_sent && out[f * 892 + k] == sent[f * 892 + k];
					as_received = as_received && out[f * 892 + k] == received[f * 892 + k];
				}
				if (e <= 16) {
					if (got != e || !as_sent) { fprintf(stderr, "case %ld: frame %llu codeword %d: %d errors, report %d, as sent %d\n", i, (unsigned long long)f, c, e, got, as_sent); bad++; }
					if (e) corrected++; else clean++;
				} else if (got == MDEMOD_RS_FAILED) {
					if (!as_received) { fprintf(stderr, "case %ld: frame %llu codeword %d: reported 255 but changed\n", i, (unsigned long long)f, c); bad++; }
					failed++;
					want_flags = MDEMOD_RS_UNCORRECTABLE;
				} else {
					fprintf(stderr, "case %ld: frame %llu codeword %d: %d errors, report %d: a false correction\n", i, (unsigned long long)f, c, e, got);
					false_corrections++; bad++;
				}
			}
			if (info[f].flags != want_flags) { fprintf(stderr, "case %ld: frame %llu: flags %u, expected %u\n", i, (unsigned long long)f, info[f].flags, want_flags); bad++; }
			mdemod_rs_header h;
			mdemod_rs_vcdu_header(out.data() + f * 892, &h);
			if (h.version > 3 || h.spacecraft > 255 || h.vcid > 63 || h.counter > 0xFFFFFFu) { fprintf(stderr, "case %ld: header out of range\n", i); bad++; }
		}
		if (n && (mdemod_rs_model_decode(&o, nullptr, n, out.data(), info.data()) != MDEMOD_ERR_PARAM || !*mdemod_last_error())) { fprintf(stderr, "case %ld: a null input was accepted\n", i); bad++; }
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"refused\": %ld, \"words\": %ld, \"clean\": %ld, \"corrected\": %ld, \"failed\": %ld, \"false_corrections\": %ld, \"bad\": %ld}\n",
	       bad ? "false" : "true", cases, refused, words, clean, corrected, failed, false_corrections, bad);
	return bad ? 1 : 0;
}
