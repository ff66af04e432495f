/*
 * fuzz_survey.cpp — mdemod_survey_plan and mdemod_survey_detect (csrc/survey_detect.cpp) over random and edge settings and
 * spectra under ASan + UBSan (tests/test_survey_host.py).  Every accepted plan is checked (fft_size a power of two in range, the
 * smallest that resolves symrate / 100 unless clamped; D divides fs and leaves 2.4 x symrate); every accepted detection is
 * checked (count within max_candidates, offsets finite and no closer to the band's edge than 0.8 symrate, strongest first,
 * best_row a row); every refusal leaves a text.  Prints one JSON line.
 * Usage: fuzz_survey <cases> <seed> <max seconds per call>
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_survey.h"

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 3000;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	const double bound = argc > 3 ? atof(argv[3]) : 2.0;
	const int rates[] = { 0, -1, 1, 7, 172800, 172799, 230000, 2048000, 2400000, 10000000, 2147483647 };
	const int syms[] = { 0, -5, 1, 9000, 72000, 80000, 1000000, 2147483647 };
	const uint32_t ffts[] = { 0, 1, 128, 255, 256, 257, 512, 1000, 1024, 2048, 4096, 8192, 16384, 32768, 0x80000000u, 0xFFFFFFFFu };
	const uint32_t rows_[] = { 0, 1, 2, 7, 8, 4096, 4097, 0xFFFFFFFFu };
	const uint32_t cands[] = { 0, 1, 2, 8, 32, 33, 0xFFFFFFFFu };
	const int bpss[] = { 0, 8, 12, 16, 32 };
	const double snrs[] = { -6.0, 0.0, -40.0, 30.0, 1e300, -1e300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity() };
	const float poison[] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
	long accepted = 0, planned = 0, bad = 0;
	double worst = 0.0;
	std::vector<float> psd;
	for (long i = 0; i < cases; i++) {
		mdemod_params in;
		memset(&in, 0, sizeof(in));
		mdemod_survey_opts o;
		mdemod_survey_default_opts(&o);
		const bool edge = (rng() & 3) == 0;
		in.samplerate = edge ? rates[rng() % (sizeof(rates) / sizeof(rates[0]))] : static_cast<int>(rng() % 12000000);
		in.symrate = edge ? syms[rng() % (sizeof(syms) / sizeof(syms[0]))] : 1000 + static_cast<int>(rng() % 150000);
		in.bps = edge ? bpss[rng() % (sizeof(bpss) / sizeof(bpss[0]))] : 8 << (rng() % 3);
		uint32_t nfft = edge ? ffts[rng() % (sizeof(ffts) / sizeof(ffts[0]))] : 256u << (rng() % 7);
		uint32_t rows = edge ? rows_[rng() % (sizeof(rows_) / sizeof(rows_[0]))] : 1 + static_cast<uint32_t>(rng() % 9);
		o.max_candidates = (rng() & 3) == 0 ? cands[rng() % (sizeof(cands) / sizeof(cands[0]))] : 1 + static_cast<uint32_t>(rng() % 32);
		o.min_snr_db = (rng() & 3) == 0 ? snrs[rng() % (sizeof(snrs) / sizeof(snrs[0]))] : -30.0 + static_cast<double>(rng() % 50);
		if ((rng() & 7) == 0) o.fft_size = ffts[rng() % (sizeof(ffts) / sizeof(ffts[0]))];
		if ((rng() & 7) == 0) o.decimation = static_cast<int32_t>(rng() % 400) - 100;

		uint32_t pf = 0;
		int32_t pd = 0;
		auto t0 = std::chrono::steady_clock::now();
		int rc = mdemod_survey_plan(&in, &pf, &pd);
		double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		if (dt > worst) worst = dt;
		if (rc != MDEMOD_OK) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) { fprintf(stderr, "case %ld: plan rc %d, text '%s'\n", i, rc, mdemod_last_error()); bad++; }
		} else {
			planned++;
			const bool pow2 = pf >= 256 && pf <= 16384 && (pf & (pf - 1)) == 0;
			const bool fine = static_cast<double>(in.samplerate) / pf <= in.symrate / 100.0;
			const bool smallest = pf == 256 || static_cast<double>(in.samplerate) / (pf / 2) > in.symrate / 100.0;
			const bool d_ok = pd >= 1 && pd <= 128 && in.samplerate % pd == 0 && (pd == 1 || static_cast<double>(in.samplerate / pd) >= 2.4 * in.symrate);
			if (!pow2 || !(fine || pf == 16384) || !smallest || !d_ok) { fprintf(stderr, "case %ld: plan fs %d sym %d -> fft %u D %d\n", i, in.samplerate, in.symrate, pf, pd); bad++; }
		}

		/* a spectrum: a floor, some humps, sometimes a value that is not finite; never larger than 2^21 floats */
		const uint64_t cells = static_cast<uint64_t>(nfft) * rows;
		const bool fits = cells > 0 && cells <= (1u << 21);
		const uint32_t an = fits ? nfft : 256, ar = fits ? rows : 1;
		psd.assign(static_cast<size_t>(an) * ar, 0.0f);
		const int kind = static_cast<int>(rng() % 8);
		for (size_t k = 0; k < psd.size(); k++) psd[k] = kind == 0 ? 0.0f : 1.0f + static_cast<float>(rng() % 1000) * 1e-3f;
		for (int h = 0; h < static_cast<int>(rng() % 5); h++) {
			const uint32_t c = static_cast<uint32_t>(rng() % an), wdt = 1 + static_cast<uint32_t>(rng() % (an / 4 + 1));
			const float amp = static_cast<float>(std::pow(10.0, static_cast<double>(rng() % 80) / 10.0 - 2.0));
			for (uint32_t r = 0; r < ar; r++)
				for (uint32_t k = 0; k < wdt; k++) psd[static_cast<size_t>(r) * an + (c + k) % an] += amp;
		}
		if (kind == 1) psd[rng() % psd.size()] = poison[rng() % 3];
		if (kind == 2) for (float &v : psd) v = 3.0e38f;
		if (!fits && (rng() & 1)) { nfft = an; rows = ar; }             /* (else: a size the entry must refuse before it reads) */
		std::vector<mdemod_survey_hit> hits(MDEMOD_SURVEY_MAX_CANDIDATES + 1);
		const uint32_t cap = static_cast<uint32_t>(rng() % (MDEMOD_SURVEY_MAX_CANDIDATES + 2));
		uint32_t n = 0xDEADBEEF;
		const bool call_ok = (static_cast<uint64_t>(nfft) * rows <= psd.size() && nfft == an) || nfft < 256 || nfft > 16384 || (nfft & (nfft - 1)) || rows < 1 || rows > 4096;
		if (!call_ok) continue;
		t0 = std::chrono::steady_clock::now();
		rc = mdemod_survey_detect(&in, (rng() & 7) ? &o : nullptr, psd.data(), nfft, rows, hits.data(), cap > MDEMOD_SURVEY_MAX_CANDIDATES ? MDEMOD_SURVEY_MAX_CANDIDATES : cap, &n);
		dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		if (dt > worst) worst = dt;
		if (dt > bound) { fprintf(stderr, "case %ld: %.3f s\n", i, dt); bad++; }
		if (rc != MDEMOD_OK) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || n != 0) { fprintf(stderr, "case %ld: detect rc %d, n %u, text '%s'\n", i, rc, n, mdemod_last_error()); bad++; }
			continue;
		}
		accepted++;
		if (n > MDEMOD_SURVEY_MAX_CANDIDATES) { fprintf(stderr, "case %ld: %u hits\n", i, n); bad++; continue; }
		const uint32_t shown = n < cap ? n : (cap > MDEMOD_SURVEY_MAX_CANDIDATES ? MDEMOD_SURVEY_MAX_CANDIDATES : cap);
		for (uint32_t k = 0; k < shown; k++) {
			const mdemod_survey_hit &h = hits[k];
			const bool ok = std::isfinite(h.coarse_offset_hz) && h.offset_hz == h.coarse_offset_hz &&
			                std::fabs(h.coarse_offset_hz) <= 0.5 * in.samplerate - 0.8 * in.symrate && std::isfinite(h.psd_snr_db) && h.best_row < rows &&
			                !h.confirmed && !h.refined && (k == 0 || h.psd_snr_db <= hits[k - 1].psd_snr_db);
			if (!ok) { fprintf(stderr, "case %ld: hit %u: offset %g snr %g row %u\n", i, k, h.coarse_offset_hz, h.psd_snr_db, h.best_row); bad++; }
		}
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"planned\": %ld, \"accepted\": %ld, \"bad\": %ld, \"worst_seconds\": %.4f}\n", bad ? "false" : "true", cases,
	       planned, accepted, bad, worst);
	return bad ? 1 : 0;
}
