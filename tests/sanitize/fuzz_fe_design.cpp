/*
 * fuzz_fe_design.cpp — mdemod_fe_design (csrc/frontend_design.cpp) over random and edge settings under ASan + UBSan
 * (tests/test_frontend_host.py).  Every accepted design is checked: length tpp * D + 1 (1 for D = 1), symmetric, sum within
 * 1e-6 of 1, the phase step llround(-offset / fs * 2^32) mod 2^32; every refusal leaves a text.  Prints one JSON line.
 * Usage: fuzz_fe_design <cases> <seed> <max seconds per call>
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_frontend.h"

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 20000;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	const double bound = argc > 3 ? atof(argv[3]) : 2.0;
	const int rates[] = { 0, -1, 1, 7, 48000, 230000, 250000, 1024000, 2048000, 2400000, 2500000, 3000000, 6000000, 10000000, 20000000, 2147483647 };
	const int syms[] = { 0, -5, 1, 9000, 72000, 80000, 1000000, 2147483647 };
	const int decs[] = { -1, 0, 1, 2, 3, 7, 8, 13, 40, 64, 127, 128, 129, 100000 };
	const int tpps[] = { -3, 0, 1, 7, 8, 16, 31, 32, 33, 1000 };
	const int bpss[] = { 0, 8, 12, 16, 32, 64 };
	const double offs[] = { 0.0, 1.0, -1.0, 300000.0, -312500.0, 1e9, -1e9, std::numeric_limits<double>::quiet_NaN(),
	                        std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), 1e-300 };
	std::vector<float> taps(MDEMOD_FE_MAX_TAPS + 8);
	long accepted = 0, bad = 0;
	double worst = 0.0;
	for (long i = 0; i < cases; i++) {
		mdemod_params in;
		memset(&in, 0, sizeof(in));
		mdemod_fe_params fe;
		memset(&fe, 0, sizeof(fe));
		const bool edge = (rng() & 3) == 0;
		in.samplerate = edge ? rates[rng() % (sizeof(rates) / sizeof(rates[0]))] : static_cast<int>(rng() % 20000000);
		in.symrate = edge ? syms[rng() % (sizeof(syms) / sizeof(syms[0]))] : static_cast<int>(rng() % 200000);
		in.bps = bpss[rng() % (sizeof(bpss) / sizeof(bpss[0]))];
		in.n_streams = 1 + static_cast<uint32_t>(rng() % 3);
		fe.decimation = edge ? decs[rng() % (sizeof(decs) / sizeof(decs[0]))] : 1 + static_cast<int>(rng() % 130);
		fe.taps_per_phase = tpps[rng() % (sizeof(tpps) / sizeof(tpps[0]))];
		double per[3];
		for (double &o : per) o = (rng() & 1) ? offs[rng() % (sizeof(offs) / sizeof(offs[0]))] : (std::ldexp(static_cast<double>(rng() >> 11), -53) - 0.5) * in.samplerate;
		fe.offset_hz = per[0];
		fe.offsets_hz = (rng() & 3) == 0 ? per : nullptr;
		if ((rng() & 1) && !edge) {                       /* half of the random draws inside the accepted region */
			fe.decimation = 1 + static_cast<int>(rng() % 128);
			in.symrate = 1000 + static_cast<int>(rng() % 150000);
			in.samplerate = fe.decimation * static_cast<int>(std::ceil(2.4 * in.symrate) + rng() % 200000);
			in.bps = 8 << (rng() % 3);
			fe.taps_per_phase = 8 + static_cast<int>(rng() % 25);
			for (double &o : per) o = (std::ldexp(static_cast<double>(rng() >> 11), -53) - 0.5) * 0.999 * in.samplerate;
			fe.offset_hz = per[0];
		}
		uint32_t n = 0, step = 0;
		const auto t0 = std::chrono::steady_clock::now();
		const int rc = mdemod_fe_design(&in, &fe, taps.data(), static_cast<uint32_t>(taps.size()), &n, &step);
		const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		if (dt > worst) worst = dt;
		if (dt > bound) { fprintf(stderr, "case %ld: %.3f s\n", i, dt); bad++; }
		if (rc != MDEMOD_OK) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) { fprintf(stderr, "case %ld: rc %d, text '%s'\n", i, rc, mdemod_last_error()); bad++; }
			continue;
		}
		accepted++;
		const int tpp = fe.taps_per_phase ? fe.taps_per_phase : MDEMOD_FE_DEFAULT_TAPS_PER_PHASE;
		const uint32_t want = fe.decimation == 1 ? 1u : static_cast<uint32_t>(tpp * fe.decimation + 1);
		double sum = 0.0;
		bool sym = true;
		for (uint32_t k = 0; k < n; k++) { sum += taps[k]; sym = sym && taps[k] == taps[n - 1 - k] && std::isfinite(taps[k]); }
		const double off0 = fe.offsets_hz ? fe.offsets_hz[0] : fe.offset_hz;
		const uint32_t want_step = static_cast<uint32_t>(static_cast<uint64_t>(llround(-off0 / in.samplerate * 4294967296.0)));
		if (n != want || !sym || std::fabs(sum - 1.0) > 1e-6 || step != want_step) {
			fprintf(stderr, "case %ld: n %u (want %u) sym %d sum %.9g step %u (want %u)\n", i, n, want, sym, sum, step, want_step);
			bad++;
		}
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"accepted\": %ld, \"bad\": %ld, \"worst_seconds\": %.4f}\n", bad ? "false" : "true", cases, accepted, bad, worst);
	return bad ? 1 : 0;
}
