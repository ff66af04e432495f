/*
 * frontend_design.cpp — the front end's settings, filter and phase steps on the host (include/meteor_demod_amd_frontend.h).
 * No HIP here: the kernels and the device entries are in frontend.hip.
 *
 * The filter: a sinc with cutoff fs_out / 2 under a Kaiser window (beta 8), L = taps_per_phase x D + 1 taps, computed in double,
 * normalised to sum 1 (unit DC gain: the baseband keeps the input format's scale for the AGC), then rounded to float.  With the
 * default 16 taps per phase and fs_out >= 3 B (B = 0.8 symrate, the edge of the RRC alpha = 0.6 spectrum): passband deviation
 * <= 0.001 dB over +-B, >= 81 dB rejection of everything that folds onto +-B (tests/test_frontend_host.py checks >= 75 dB from
 * the float taps).  At fs_out = 2.8 B the rejection drops to 56 dB, at 2.4 B to 24 dB: fs_out < 3 B (fs / D < 2.4 symrate) is
 * refused.
 */
#include <cmath>
#include <cstdint>
#include <vector>

#include "frontend_design.h"
#include "mdemod_internal_api.h"

namespace {

/* modified Bessel function of the first kind, order 0, by its power series (all terms positive: no cancellation) */
double
bessel_i0(double x)
{
	const double q = 0.25 * x * x;
	double term = 1.0, sum = 1.0;
	for (int m = 1; m < 500; m++) {
		term *= q / (static_cast<double>(m) * m);
		sum += term;
		if (term < sum * 1e-17) break;
	}
	return sum;
}

const double kPi = 3.14159265358979323846;
const double kKaiserBeta = 8.0;

} /* namespace */

uint32_t
mdemod_fe_phase_step(double offset_hz, int32_t samplerate)
{
	const long long w = llround(-offset_hz / static_cast<double>(samplerate) * 4294967296.0);
	return static_cast<uint32_t>(static_cast<uint64_t>(w));
}

int
mdemod_fe_design_host(const mdemod_params &in, const mdemod_fe_params &fe, FeDesign &out)
{
	const int32_t d = fe.decimation;
	const int32_t tpp = fe.taps_per_phase == 0 ? MDEMOD_FE_DEFAULT_TAPS_PER_PHASE : fe.taps_per_phase;
	if (d < 1 || d > MDEMOD_FE_MAX_DECIMATION) REFUSE("front end: decimation %d must be 1..%d", d, MDEMOD_FE_MAX_DECIMATION);
	if (tpp < MDEMOD_FE_MIN_TAPS_PER_PHASE || tpp > MDEMOD_FE_MAX_TAPS_PER_PHASE)
		REFUSE("front end: taps_per_phase %d must be %d..%d", tpp, MDEMOD_FE_MIN_TAPS_PER_PHASE, MDEMOD_FE_MAX_TAPS_PER_PHASE);
	if (in.samplerate <= 0 || in.symrate <= 0) REFUSE("front end: sample rate %d and symbol rate %d must be positive", in.samplerate, in.symrate);
	if (in.bps != 8 && in.bps != 16 && in.bps != 32) REFUSE("front end: %d bits per sample (8, 16 or 32 expected)", in.bps);
	if (in.samplerate % d != 0)
		REFUSE("front end: decimation %d does not divide the sample rate %d (the demodulator's sample rate is an integer)", d, in.samplerate);
	const int32_t fs_out = in.samplerate / d;
	if (d >= 2 && static_cast<double>(fs_out) < 2.4 * in.symrate)
		REFUSE("front end: decimation %d leaves %d S/s, less than 2.4 x the symbol rate %d (%.0f S/s): the anti-alias filter needs "
		       "fs / D >= 3 x 0.8 symrate", d, fs_out, in.symrate, 2.4 * in.symrate);
	const uint32_t n_streams = in.n_streams ? in.n_streams : 1;
	out.steps.assign(n_streams, 0);
	for (uint32_t s = 0; s < n_streams; s++) {
		const double off = fe.offsets_hz ? fe.offsets_hz[s] : fe.offset_hz;
		if (!std::isfinite(off)) REFUSE("front end: offset of stream %u is not a finite number of Hz", s);
		if (!(std::fabs(off) < 0.5 * in.samplerate))
			REFUSE("front end: offset %.1f Hz of stream %u is not inside +-fs/2 = +-%.1f Hz", off, s, 0.5 * in.samplerate);
		out.steps[s] = mdemod_fe_phase_step(off, in.samplerate);
	}
	out.decimation = d;
	out.taps_per_phase = tpp;
	out.samplerate_out = fs_out;
	if (d == 1) {
		out.n_taps = 1;
		out.taps.assign(1, 1.0f);
		return MDEMOD_OK;
	}
	const uint32_t L = static_cast<uint32_t>(tpp) * static_cast<uint32_t>(d) + 1;
	const uint32_t H = L - 1;                                     /* even: the centre tap is H / 2 */
	std::vector<double> h(L);
	const double i0b = bessel_i0(kKaiserBeta);
	for (uint32_t k = 0; k <= H / 2; k++) {                      /* one half, mirrored: the taps are symmetric bit for bit */
		const double t = static_cast<double>(static_cast<int64_t>(k) - static_cast<int64_t>(H / 2)) / d;   /* in output samples */
		const double sinc = t == 0.0 ? 1.0 : std::sin(kPi * t) / (kPi * t);
		const double r = 2.0 * k / H - 1.0;
		const double w = bessel_i0(kKaiserBeta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
		h[k] = h[H - k] = sinc * w;
	}
	double sum = 0.0;
	for (uint32_t k = 0; k < L; k++) sum += h[k];
	out.n_taps = L;
	out.taps.resize(L);
	for (uint32_t k = 0; k < L; k++) out.taps[k] = static_cast<float>(h[k] / sum);
	return MDEMOD_OK;
}

extern "C" int
mdemod_fe_design(const mdemod_params *input, const mdemod_fe_params *fe, float *taps, uint32_t cap, uint32_t *n_taps, uint32_t *step)
try { MDEMOD_API_ENTER
	if (!input || !fe) { mdm_note_error("mdemod_fe_design: input and fe are needed"); return MDEMOD_ERR_PARAM; }
	FeDesign d;
	const int rc = mdemod_fe_design_host(*input, *fe, d);
	if (rc) return rc;
	if (taps) {
		if (cap < d.n_taps) { mdm_note_error("mdemod_fe_design: %u taps do not fit a buffer of %u", d.n_taps, cap); return MDEMOD_ERR_PARAM; }
		for (uint32_t k = 0; k < d.n_taps; k++) taps[k] = d.taps[k];
	}
	if (n_taps) *n_taps = d.n_taps;
	if (step) *step = d.steps[0];
	return MDEMOD_OK;
} MDEMOD_API_CATCH
