/*
 * interleave_host.cpp — host side of the 80 k interleaved mode (include/meteor_demod_amd_interleave.h): the sync word's pattern,
 * the tracker that serves the product and the model alike, and the host model of the two kernels of csrc/interleave.hip
 * (mdemod_il_model_*: the kernels' specification, written for reading, one core, plain loops).  HIP-free.
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "frames_host.h"
#include "interleave_host.h"
#include "mdemod_internal_api.h"

namespace {

/* rail `rail` (0: I", 1: Q") of symbol i of soft[m][2] through the combined hypothesis H = h + 8 s, in int32: I' and Q' are the
 * stream through h; s = 1 reads (I'[i], Q'[i + 1]), s = 2 (I'[i + 1], Q'[i]); a rail value at index m and beyond is 0 */
inline int
rail_through(const int8_t *soft, uint64_t m, uint64_t i, uint32_t H, uint32_t rail)
{
	const FrHyp y = fr_hyp(H & 7u);
	const uint32_t s = H >> 3;
	if (rail == 0) {
		const uint64_t ii = i + (s == 2);
		return ii < m ? y.si * soft[2 * ii + (y.swap ? 1 : 0)] : 0;
	}
	const uint64_t qi = i + (s == 1);
	return qi < m ? y.sq * soft[2 * qi + (y.swap ? 0 : 1)] : 0;
}

} /* namespace */

void
il_pattern(int8_t a[IL_SYNC], int8_t b[IL_SYNC])
{
	const uint32_t word = 0x27;                                              /* MSB first: symbol i is (bit 2 i, bit 2 i + 1) */
	for (uint32_t i = 0; i < IL_SYNC; i++) {
		a[i] = (word >> (7 - 2 * i)) & 1u ? 1 : -1;
		b[i] = (word >> (6 - 2 * i)) & 1u ? 1 : -1;
	}
}

int
il_settings(const mdemod_il_opts *opts, mdemod_il_opts &out)
{
	mdemod_il_default_opts(&out);
	if (!opts) return MDEMOD_OK;
	if (opts->branch_delay == 0) REFUSE("interleave: branch_delay 0 (the branch delay M is at least 1)");
	if (opts->min_run == 0) REFUSE("interleave: min_run 0 (a run counts from at least one window)");
	if (opts->reserved[0] || opts->reserved[1]) REFUSE("interleave: the reserved words of mdemod_il_opts must be 0");
	out = *opts;
	return MDEMOD_OK;
}

int
il_check_candidates(const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m)
{
	if (n_windows != il_windows(m))
		REFUSE("interleave: %llu candidates for %llu symbols (there are %llu windows)", (unsigned long long)n_windows, (unsigned long long)m,
		       (unsigned long long)il_windows(m));
	for (uint64_t w = 0; w < n_windows; w++) {
		const uint64_t p = cand[w].position;
		if (p / IL_WINDOW != w || p - w * IL_WINDOW >= IL_PERIOD || p > m - IL_SYNC)
			REFUSE("interleave: candidate %llu stands at %llu, outside its window's 40 phases (or past the last position)", (unsigned long long)w,
			       (unsigned long long)p);
		if (cand[w].hypothesis >= IL_HYPS) REFUSE("interleave: candidate %llu has hypothesis %u (there are 24)", (unsigned long long)w, cand[w].hypothesis);
	}
	return MDEMOD_OK;
}

int
il_check_segments(const mdemod_il_segment *segments, uint64_t n_segments, uint64_t n_periods, uint64_t m)
{
	if (m >> 48) REFUSE("interleave: a stream of %llu symbols is more than the layer takes", (unsigned long long)m);
	if (n_periods > m) REFUSE("interleave: %llu periods in %llu symbols", (unsigned long long)n_periods, (unsigned long long)m);
	if (n_periods && !n_segments) REFUSE("interleave: %llu periods but no segment", (unsigned long long)n_periods);
	for (uint64_t i = 0; i < n_segments; i++) {
		const mdemod_il_segment &s = segments[i];
		if (i == 0 ? s.period != 0 : s.period < segments[i - 1].period)
			REFUSE("interleave: segment %llu begins at period %llu (the first begins at 0, and periods do not descend)", (unsigned long long)i,
			       (unsigned long long)s.period);
		if (s.hypothesis >= IL_HYPS) REFUSE("interleave: segment %llu has hypothesis %u (there are 24)", (unsigned long long)i, s.hypothesis);
		if (s.marker_symbol > m) REFUSE("interleave: segment %llu has its sync word at %llu of %llu symbols", (unsigned long long)i,
		                                (unsigned long long)s.marker_symbol, (unsigned long long)m);
	}
	return MDEMOD_OK;
}

void
il_track(const mdemod_il_opts &o, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m, std::vector<mdemod_il_segment> &segments,
         uint64_t &n_periods)
{
	segments.clear();
	for (uint64_t w = 0; w < n_windows;) {
		const uint32_t r = static_cast<uint32_t>(cand[w].position - w * IL_WINDOW), H = cand[w].hypothesis;
		uint64_t e = w + 1;
		while (e < n_windows && cand[e].position - e * IL_WINDOW == r && cand[e].hypothesis == H) e++;
		const bool counts = e - w >= o.min_run;
		if (counts && (segments.empty() || segments.back().phase != r || segments.back().hypothesis != H)) {
			mdemod_il_segment s;
			s.first_symbol = segments.empty() ? 0 : w * IL_WINDOW;
			s.marker_symbol = s.first_symbol + r;                             /* (the first symbol is a multiple of 40) */
			s.period = segments.empty() ? 0 : segments.back().period + (s.marker_symbol - segments.back().marker_symbol + IL_PERIOD / 2) / IL_PERIOD;
			s.phase = r;
			s.hypothesis = H;
			segments.push_back(s);
		}
		w = e;
	}
	n_periods = segments.empty() ? 0 : segments.back().period + (m - segments.back().marker_symbol) / IL_PERIOD;
}

int32_t
il_mean_score(const mdemod_frames_candidate *cand, uint64_t n_windows)
{
	int64_t sum = 0;
	for (uint64_t w = 0; w < n_windows; w++) sum += cand[w].score;
	return n_windows ? static_cast<int32_t>(sum / static_cast<int64_t>(n_windows)) : 0;
}

extern "C" {

void
mdemod_il_default_opts(mdemod_il_opts *opts)
{
	if (!opts) return;
	opts->branch_delay = MDEMOD_IL_DEFAULT_BRANCH_DELAY;
	opts->min_run = MDEMOD_IL_DEFAULT_MIN_RUN;
	opts->reserved[0] = opts->reserved[1] = 0;
}

uint64_t
mdemod_il_windows(uint64_t m)
{
	return il_windows(m);
}

uint64_t
mdemod_il_max_output_symbols(uint64_t m)
{
	return IL_BRANCHES * (m / IL_PERIOD) + IL_BRANCHES;
}

int
mdemod_il_track(const mdemod_il_opts *opts, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m, mdemod_il_segment *segments,
                uint64_t cap, uint64_t *n_segments, uint64_t *n_periods)
try { MDEMOD_API_ENTER
	if (n_segments) *n_segments = 0;
	if (n_periods) *n_periods = 0;
	if (!n_segments || !n_periods || (n_windows && !cand) || (cap && !segments))
		REFUSE("mdemod_il_track: the candidates, n_segments and n_periods (and segments for cap > 0) are needed");
	mdemod_il_opts o;
	int rc;
	if ((rc = il_settings(opts, o)) || (rc = il_check_candidates(cand, n_windows, m))) return rc;
	std::vector<mdemod_il_segment> found;
	il_track(o, cand, n_windows, m, found, *n_periods);
	*n_segments = found.size();
	for (uint64_t i = 0; i < found.size() && i < cap; i++) segments[i] = found[i];
	return MDEMOD_OK;
} MDEMOD_API_CATCH

/* ------------------------------------------------------------------------------------------------------------ the model */

void
mdemod_il_model_pattern(int8_t *a, int8_t *b)
{
	il_pattern(a, b);
}

int
mdemod_il_model_candidates(const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand)
try { MDEMOD_API_ENTER
	const uint64_t n_windows = il_windows(m);
	if (n_windows && (!soft || !cand)) REFUSE("mdemod_il_model_candidates: the symbols and the candidates are needed");
	int8_t a[IL_SYNC], b[IL_SYNC];
	il_pattern(a, b);
	for (uint64_t w = 0; w < n_windows; w++) {
		const uint64_t first = w * IL_WINDOW, end = std::min<uint64_t>(first + IL_WINDOW, m - (IL_SYNC - 1));   /* positions [first, end) */
		bool have = false;
		mdemod_frames_candidate best = { 0, 0, 0 };
		for (uint32_t r = 0; r < IL_PERIOD && first + r < end; r++)
			for (uint32_t H = 0; H < IL_HYPS; H++) {
				int32_t sum = 0;
				for (uint64_t p = first + r; p < end; p += IL_PERIOD)
					for (uint32_t i = 0; i < IL_SYNC; i++) sum += a[i] * rail_through(soft, m, p + i, H, 0) + b[i] * rail_through(soft, m, p + i, H, 1);
				if (!have || sum > best.score) {                              /* equal: the lowest r, then the lowest H, stands */
					best.position = first + r; best.hypothesis = H; best.score = sum;
					have = true;
				}
			}
		cand[w] = best;
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_il_model_deinterleave(const mdemod_il_opts *opts, const int8_t *soft, uint64_t m, const mdemod_il_segment *segments, uint64_t n_segments,
                             uint64_t n_periods, int8_t *out)
try { MDEMOD_API_ENTER
	mdemod_il_opts o;
	int rc;
	if ((rc = il_settings(opts, o))) return rc;
	if ((m && !soft) || (n_segments && !segments) || (n_periods && !out)) REFUSE("mdemod_il_model_deinterleave: the symbols, the segments and the output are needed");
	if ((rc = il_check_segments(segments, n_segments, n_periods, m))) return rc;
	const uint64_t step = static_cast<uint64_t>(IL_BRANCHES) * o.branch_delay;
	for (uint64_t k = 0; k < IL_DATA_BITS * n_periods; k++) {
		const uint64_t kp = k + step * (k % IL_BRANCHES), N = kp / IL_DATA_BITS, j = kp % IL_DATA_BITS;
		if (N >= n_periods) { out[k] = 0; continue; }
		uint64_t i = 0;
		while (i + 1 < n_segments && segments[i + 1].period <= N) i++;      /* the last segment with N0 <= N */
		const uint64_t x = segments[i].marker_symbol + IL_PERIOD * (N - segments[i].period) + IL_SYNC + j / 2;
		const int v = rail_through(soft, m, x, segments[i].hypothesis, static_cast<uint32_t>(j & 1u));
		out[k] = static_cast<int8_t>(v > 127 ? 127 : v);
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
