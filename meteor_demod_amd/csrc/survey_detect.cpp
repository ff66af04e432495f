/*
 * survey_detect.cpp — the survey's settings, plan and detector on the host (include/meteor_demod_amd_survey.h).
 * No HIP here: the spectrum kernels and the device entries are in survey.hip.
 *
 * The detector: P = the rows' sum (double), floor = its median (signals cover a minority of a band that is worth surveying),
 * c[k] = sum over m of (P[k + m] - floor) t[m], circular, with t the raised-cosine POWER response of a signal of symrate with
 * roll-off 0.6 (1 inside (1 - a) / 2 symrate, 0 outside (1 + a) / 2 symrate = 0.8 symrate).  t is short (1.6 symrate of bins),
 * so the correlation is done directly.  Peaks are taken strongest first; each suppresses +-1.6 symrate around itself; a peak's
 * position is interpolated by a parabola through c[k - 1], c[k], c[k + 1]; matched power over the floor = c[k] / sum t / floor.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "survey_detect.h"
#include "mdemod_internal_api.h"

namespace {

const double kPi = 3.14159265358979323846;

int
check_rates(const mdemod_params &p)
{
	if (p.samplerate <= 0 || p.symrate <= 0) REFUSE("survey: sample rate %d and symbol rate %d must be positive", p.samplerate, p.symrate);
	if (p.bps != 8 && p.bps != 16 && p.bps != 32) REFUSE("survey: %d bits per sample (8, 16 or 32 expected)", p.bps);
	if (static_cast<double>(p.samplerate) < 2.4 * p.symrate)
		REFUSE("survey: the sample rate %d is less than 2.4 x the symbol rate %d: the recording is no wider than the signal, there is "
		       "nothing to survey", p.samplerate, p.symrate);
	return MDEMOD_OK;
}

void
plan(const mdemod_params &p, uint32_t &fft_size, int32_t &decimation)
{
	uint32_t n = MDEMOD_SURVEY_MIN_FFT;
	while (n < MDEMOD_SURVEY_MAX_FFT && static_cast<double>(p.samplerate) / n > p.symrate / 100.0) n *= 2;
	fft_size = n;
	decimation = 1;
	for (int32_t d = MDEMOD_FE_MAX_DECIMATION; d >= 2; d--)
		if (p.samplerate % d == 0 && static_cast<double>(p.samplerate / d) >= 2.4 * p.symrate) { decimation = d; break; }
}

} /* namespace */

bool
mdemod_survey_fft_size_ok(uint32_t n)
{
	return n >= MDEMOD_SURVEY_MIN_FFT && n <= MDEMOD_SURVEY_MAX_FFT && (n & (n - 1)) == 0;
}

int
mdemod_survey_settings(const mdemod_params &p, const mdemod_survey_opts *o, SurveySettings &s)
{
	int rc = check_rates(p);
	if (rc) return rc;
	mdemod_survey_opts d;
	mdemod_survey_default_opts(&d);
	if (o) d = *o;
	plan(p, s.fft_size, s.decimation);
	if (d.fft_size) {
		if (!mdemod_survey_fft_size_ok(d.fft_size))
			REFUSE("survey: fft_size %u must be a power of two, %d..%d", d.fft_size, MDEMOD_SURVEY_MIN_FFT, MDEMOD_SURVEY_MAX_FFT);
		s.fft_size = d.fft_size;
	}
	s.n_rows = d.n_rows ? d.n_rows : MDEMOD_SURVEY_DEFAULT_ROWS;
	if (s.n_rows > MDEMOD_SURVEY_MAX_ROWS) REFUSE("survey: n_rows %u must be 1..%d", s.n_rows, MDEMOD_SURVEY_MAX_ROWS);
	s.max_candidates = d.max_candidates ? d.max_candidates : MDEMOD_SURVEY_DEFAULT_CANDIDATES;
	if (s.max_candidates > MDEMOD_SURVEY_MAX_CANDIDATES)
		REFUSE("survey: max_candidates %u must be 1..%d", s.max_candidates, MDEMOD_SURVEY_MAX_CANDIDATES);
	if (!std::isfinite(d.min_snr_db)) REFUSE("survey: min_snr_db is not a finite number of dB");
	s.min_snr_db = d.min_snr_db;
	if (d.decimation) {
		if (d.decimation < 1 || d.decimation > MDEMOD_FE_MAX_DECIMATION) REFUSE("survey: decimation %d must be 1..%d", d.decimation, MDEMOD_FE_MAX_DECIMATION);
		s.decimation = d.decimation;             /* (whether it fits fs and symrate is mdemod_fe_design's to say) */
	}
	if (!(d.clock_threshold >= 0.0f) || !std::isfinite(d.clock_threshold)) REFUSE("survey: clock_threshold must be a finite number >= 0");
	if (!(d.carrier_threshold >= 0.0f) || !std::isfinite(d.carrier_threshold)) REFUSE("survey: carrier_threshold must be a finite number >= 0");
	s.clock_threshold = d.clock_threshold > 0.0f ? d.clock_threshold : MDEMOD_SURVEY_CLOCK_THRESHOLD;
	s.carrier_threshold = d.carrier_threshold > 0.0f ? d.carrier_threshold : MDEMOD_SURVEY_CARRIER_THRESHOLD;
	return MDEMOD_OK;
}

int
mdemod_survey_detect_host(const mdemod_params &p, const SurveySettings &s, const float *psd, uint32_t N, uint32_t n_rows,
                          std::vector<mdemod_survey_hit> &hits)
{
	hits.clear();
	const double fs = p.samplerate, sym = p.symrate, bin = fs / N;
	std::vector<double> P(N, 0.0);
	for (uint32_t r = 0; r < n_rows; r++)
		for (uint32_t k = 0; k < N; k++) {
			const float v = psd[static_cast<size_t>(r) * N + k];
			if (!std::isfinite(v)) REFUSE("survey: the spectrum holds a value that is not finite (row %u, bin %u)", r, k);
			P[k] += v;
		}
	std::vector<double> sorted(P);
	std::nth_element(sorted.begin(), sorted.begin() + N / 2, sorted.end());
	const double floor = sorted[N / 2];
	if (!(floor > 0.0) || !std::isfinite(floor)) return MDEMOD_OK;          /* an empty spectrum: nothing stands out of nothing */

	/* the matched shape, bins -M .. M */
	const double alpha = MDEMOD_SURVEY_ROLLOFF;
	const int M = std::min(static_cast<int>(0.5 * (1.0 + alpha) * sym / bin), static_cast<int>(N / 2) - 1);
	std::vector<double> t(2 * M + 1);
	double tsum = 0.0;
	for (int m = -M; m <= M; m++) {
		const double a = std::fabs(m * bin) / sym;
		double v = 0.0;
		if (a <= 0.5 * (1.0 - alpha)) v = 1.0;
		else if (a < 0.5 * (1.0 + alpha)) v = 0.5 * (1.0 + std::cos(kPi / alpha * (a - 0.5 * (1.0 - alpha))));
		t[m + M] = v;
		tsum += v;
	}
	std::vector<double> c(N);
	for (uint32_t k = 0; k < N; k++) {
		double acc = 0.0;
		for (int m = -M; m <= M; m++) acc += (P[(k + N + m) & (N - 1)] - floor) * t[m + M];
		c[k] = acc;
	}
	const int w = static_cast<int>(1.6 * sym / bin);
	std::vector<char> dead(N, 0);
	for (uint32_t n = 0; n < s.max_candidates; n++) {
		int64_t k = -1;
		for (uint32_t i = 0; i < N; i++)
			if (!dead[i] && (k < 0 || c[i] > c[k])) k = i;
		if (k < 0 || !(c[k] > 0.0)) break;
		const double snr_db = 10.0 * std::log10(c[k] / tsum / floor);
		if (snr_db < s.min_snr_db) break;                                   /* (what is left is weaker still) */
		const double a = c[(k + N - 1) & (N - 1)], b = c[k], d = c[(k + 1) & (N - 1)];
		const double den = a - 2.0 * b + d;
		double frac = den != 0.0 ? 0.5 * (a - d) / den : 0.0;
		if (!(frac >= -0.5 && frac <= 0.5)) frac = 0.0;                     /* (a neighbour inside a suppressed stretch may be larger) */
		for (int m = -w; m <= w && m < static_cast<int>(N) - w; m++) dead[(k + N + m) & (N - 1)] = 1;
		const double coarse = (static_cast<double>(k) - N / 2 + frac) * bin;
		if (std::fabs(coarse) > 0.5 * fs - 0.8 * sym) continue;             /* too close to the band's edge for the front end's filter */
		mdemod_survey_hit h;
		h.offset_hz = h.coarse_offset_hz = coarse;
		h.psd_snr_db = static_cast<float>(snr_db);
		h.clock_quality = h.carrier_quality = 0.0f;
		h.confirmed = h.refined = 0;
		h.best_row = 0;
		double best = 0.0;
		for (uint32_t r = 0; r < n_rows; r++) {
			double acc = 0.0;
			for (int m = -M; m <= M; m++) acc += psd[static_cast<size_t>(r) * N + ((k + N + m) & (N - 1))] * t[m + M];
			if (r == 0 || acc > best) { best = acc; h.best_row = r; }
		}
		hits.push_back(h);
	}
	return MDEMOD_OK;
}

extern "C" void
mdemod_survey_default_opts(mdemod_survey_opts *o)
{
	if (!o) return;
	o->fft_size = 0;
	o->n_rows = MDEMOD_SURVEY_DEFAULT_ROWS;
	o->max_candidates = MDEMOD_SURVEY_DEFAULT_CANDIDATES;
	o->decimation = 0;
	o->min_snr_db = MDEMOD_SURVEY_DEFAULT_MIN_SNR_DB;
	o->clock_threshold = 0.0f;
	o->carrier_threshold = 0.0f;
}

extern "C" int
mdemod_survey_plan(const mdemod_params *params, uint32_t *fft_size, int32_t *decimation)
try { MDEMOD_API_ENTER
	if (!params) REFUSE("mdemod_survey_plan: params is needed");
	const int rc = check_rates(*params);
	if (rc) return rc;
	uint32_t n;
	int32_t d;
	plan(*params, n, d);
	if (fft_size) *fft_size = n;
	if (decimation) *decimation = d;
	return MDEMOD_OK;
} MDEMOD_API_CATCH

extern "C" int
mdemod_survey_detect(const mdemod_params *params, const mdemod_survey_opts *opts, const float *psd, uint32_t fft_size, uint32_t n_rows,
                     mdemod_survey_hit *hits, uint32_t cap, uint32_t *n_hits)
try { MDEMOD_API_ENTER
	if (!params || !psd || !n_hits || (cap && !hits)) REFUSE("mdemod_survey_detect: params, psd, n_hits (and hits for cap > 0) are needed");
	*n_hits = 0;
	SurveySettings s;
	int rc = mdemod_survey_settings(*params, opts, s);
	if (rc) return rc;
	if (!mdemod_survey_fft_size_ok(fft_size))
		REFUSE("survey: fft_size %u must be a power of two, %d..%d", fft_size, MDEMOD_SURVEY_MIN_FFT, MDEMOD_SURVEY_MAX_FFT);
	if (n_rows < 1 || n_rows > MDEMOD_SURVEY_MAX_ROWS) REFUSE("survey: n_rows %u must be 1..%d", n_rows, MDEMOD_SURVEY_MAX_ROWS);
	std::vector<mdemod_survey_hit> found;
	rc = mdemod_survey_detect_host(*params, s, psd, fft_size, n_rows, found);
	if (rc) return rc;
	*n_hits = static_cast<uint32_t>(found.size());
	for (uint32_t i = 0; i < found.size() && i < cap; i++) hits[i] = found[i];
	return MDEMOD_OK;
} MDEMOD_API_CATCH
