/*
 * frames_host.cpp — host side of the frame layer (include/meteor_demod_amd_frames.h): the pattern, the tracker that serves the
 * product, and the host model of the two kernels of csrc/frames.hip (mdemod_frames_model_*: the kernels' specification, written
 * for reading, one core, no tricks).  The arithmetic takes a mode (FrMode: differential, skew) for the link variant, whose
 * entries are in csrc/frames_link_host.cpp; with both switches off it is the plain layer's.  HIP-free.
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "frames_host.h"
#include "mdemod_internal_api.h"

namespace {

inline uint32_t
parity(uint32_t x)
{
	x ^= x >> 4; x ^= x >> 2; x ^= x >> 1;
	return x & 1u;
}

inline uint32_t enc_step(uint32_t reg, uint32_t bit) { return ((reg << 1) | bit) & 0x7Fu; }
inline int enc_c1(uint32_t reg) { return parity(reg & 0x4Fu) ? 1 : -1; }
inline int enc_c2(uint32_t reg) { return parity(reg & 0x6Du) ? 1 : -1; }

/* symbol i of soft[m][2] through the combined hypothesis H = h + 8 s, in int32: I' and Q' are the stream through h; s = 1 reads
 * (I'[i], Q'[i + 1]), s = 2 (I'[i + 1], Q'[i]); a rail value at index m is 0 */
inline void
through(const int8_t *soft, uint64_t m, uint64_t i, uint32_t H, int &ip, int &qp)
{
	const FrHyp y = fr_hyp(H & 7u);
	const uint32_t s = H >> 3;
	const uint64_t ii = i + (s == 2), qi = i + (s == 1);
	ip = ii < m ? y.si * soft[2 * ii + (y.swap ? 1 : 0)] : 0;
	qp = qi < m ? y.sq * soft[2 * qi + (y.swap ? 0 : 1)] : 0;
}

/* one sub-block of the model: 1024 bits of frame `fr`, sub-block k, into out[128]; the decoder's own bits d into dbits[128] as
 * well (they are `out` unless diff: then out holds d[t] xor d[t - 1], and 0 stands for the bit before step 0) */
void
model_sub_block(const int8_t *soft, uint64_t m, const mdemod_frame_info &fr, int k, bool diff, uint8_t *out, uint8_t *dbits)
{
	const uint64_t s = fr.position + static_cast<uint64_t>(FR_SUB) * k;
	const uint64_t lo = s >= FR_HALO ? s - FR_HALO : 0, hi = std::min<uint64_t>(m, s + FR_SUB + FR_HALO);
	const uint32_t T = static_cast<uint32_t>(hi - lo), off = static_cast<uint32_t>(s - lo);
	int32_t pm[64], nx[64];
	uint64_t dec[FR_STEPS];
	for (int i = 0; i < 64; i++) pm[i] = 0;
	for (uint32_t t = 0; t < T; t++) {
		int ip, qp;
		through(soft, m, lo + t, fr.hypothesis, ip, qp);
		uint64_t word = 0;
		for (uint32_t ns = 0; ns < 64; ns++) {
			const uint32_t bit = ns & 1u, p0 = ns >> 1, p1 = (ns >> 1) | 32u;
			const uint32_t r0 = enc_step(p0, bit), r1 = enc_step(p1, bit);
			const int32_t m0 = pm[p0] + ip * enc_c1(r0) + qp * enc_c2(r0);
			const int32_t m1 = pm[p1] + ip * enc_c1(r1) + qp * enc_c2(r1);
			const bool second = m1 > m0;                                  /* equal: s' >> 1 wins */
			nx[ns] = second ? m1 : m0;
			word |= static_cast<uint64_t>(second) << ns;
		}
		dec[t] = word;
		memcpy(pm, nx, sizeof pm);
	}
	uint32_t state = 0;
	for (uint32_t i = 1; i < 64; i++)
		if (pm[i] > pm[state]) state = i;                                 /* ties: the lowest state */
	memset(out, 0, FR_SUB / 8);
	memset(dbits, 0, FR_SUB / 8);
	for (uint32_t t = T; t-- > 0;) {
		if (t >= off && t < off + FR_SUB) {
			const uint32_t j = t - off, d = state & 1u, before = t ? (state >> 1) & 1u : 0u;   /* (bit 1 of the state: the bit of step t - 1) */
			if (d) dbits[j >> 3] |= static_cast<uint8_t>(0x80u >> (j & 7u));
			if (diff ? d ^ before : d) out[j >> 3] |= static_cast<uint8_t>(0x80u >> (j & 7u));
		}
		const uint32_t d = static_cast<uint32_t>(dec[t] >> state) & 1u;
		state = (state >> 1) | (d << 5);
	}
}

uint32_t
model_channel_errors(const int8_t *soft, uint64_t m, const mdemod_frame_info &fr, const uint8_t *cadu)
{
	uint32_t reg = 0, errors = 0;
	for (uint32_t n = 0; n < FR_FRAME; n++) {
		reg = enc_step(reg, (cadu[n >> 3] >> (7 - (n & 7u))) & 1u);
		if (n < FR_LEAD) continue;
		int ip, qp;
		through(soft, m, fr.position + n, fr.hypothesis, ip, qp);
		errors += (ip > 0) != (enc_c1(reg) > 0);
		errors += (qp > 0) != (enc_c2(reg) > 0);
	}
	return errors;
}

} /* namespace */

void
fr_pattern(int8_t a[FR_TAPS], int8_t b[FR_TAPS])
{
	static const uint8_t marker[4] = { 0x1A, 0xCF, 0xFC, 0x1D };
	int8_t sym[64];
	(void)mdemod_frames_model_encode(marker, 4, 0, sym);
	for (int k = 0; k < FR_TAPS; k++) { a[k] = sym[2 * (FR_LEAD + k)]; b[k] = sym[2 * (FR_LEAD + k) + 1]; }
}

void
fr_pattern_diff(int8_t a[FR_TAPS], int8_t b[FR_TAPS])
{
	static const uint8_t marker[4] = { 0x1A, 0xCF, 0xFC, 0x1D };
	uint8_t coded[4] = { 0, 0, 0, 0 };
	uint32_t d = 0;                                                          /* d[-1] */
	for (int t = 0; t < 32; t++) {
		d ^= (marker[t >> 3] >> (7 - (t & 7))) & 1u;
		coded[t >> 3] |= static_cast<uint8_t>(d << (7 - (t & 7)));
	}
	int8_t sym[64];
	(void)mdemod_frames_model_encode(coded, 4, 0, sym);
	for (int k = 0; k < FR_TAPS; k++) { a[k] = sym[2 * (FR_LEAD + k)]; b[k] = sym[2 * (FR_LEAD + k) + 1]; }
}

int
fr_mode_of(const mdemod_frames_link *link, FrMode &md)
{
	md.diff = md.skew = false;
	if (!link) return MDEMOD_OK;
	if (link->differential > 1 || link->skew > 1) REFUSE("frames: link switches are 0 or 1 (differential %u, skew %u)", link->differential, link->skew);
	if (link->reserved[0] || link->reserved[1]) REFUSE("frames: the reserved words of mdemod_frames_link must be 0");
	md.diff = link->differential != 0;
	md.skew = link->skew != 0;
	return MDEMOD_OK;
}

int
fr_check_frames(const mdemod_frame_info *frames, uint64_t n_frames, uint64_t m, FrMode md)
{
	for (uint64_t f = 0; f < n_frames; f++) {
		if (frames[f].hypothesis >= fr_mode_hyps(md))
			REFUSE("frames: frame %llu has hypothesis %u (0..%u)", (unsigned long long)f, frames[f].hypothesis, fr_mode_hyps(md) - 1);
		if (!fr_mode_allows(frames[f].hypothesis, md))
			REFUSE("frames: frame %llu has hypothesis %u, which is outside the differential set (h in 0, 1, 4, 5)", (unsigned long long)f, frames[f].hypothesis);
		if (frames[f].position > m || m - frames[f].position < FR_FRAME)
			REFUSE("frames: frame %llu at symbol %llu is not complete in a stream of %llu symbols", (unsigned long long)f,
			       (unsigned long long)frames[f].position, (unsigned long long)m);
	}
	return MDEMOD_OK;
}

int
fr_check_candidates(const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m, FrMode md)
{
	if (n_windows != fr_mode_windows(m, md))
		REFUSE("frames: %llu candidates for a stream of %llu symbols, which has %llu windows", (unsigned long long)n_windows,
		       (unsigned long long)m, (unsigned long long)fr_mode_windows(m, md));
	for (uint64_t w = 0; w < n_windows; w++) {
		if (cand[w].hypothesis >= fr_mode_hyps(md))
			REFUSE("frames: candidate %llu has hypothesis %u (0..%u)", (unsigned long long)w, cand[w].hypothesis, fr_mode_hyps(md) - 1);
		if (!fr_mode_allows(cand[w].hypothesis, md))
			REFUSE("frames: candidate %llu has hypothesis %u, which is outside the differential set (h in 0, 1, 4, 5)", (unsigned long long)w, cand[w].hypothesis);
		if (cand[w].position / FR_FRAME != w || cand[w].position >= m - fr_mode_span(md))
			REFUSE("frames: candidate %llu at symbol %llu is outside its window", (unsigned long long)w, (unsigned long long)cand[w].position);
	}
	return MDEMOD_OK;
}

/* the candidates under a mode, as the specification words them: every allowed H of every position, the symbols taken through H */
void
fr_model_candidates(const int8_t *soft, uint64_t m, FrMode md, mdemod_frames_candidate *cand)
{
	const uint64_t n_windows = fr_mode_windows(m, md), span = fr_mode_span(md);
	int8_t a[FR_TAPS], b[FR_TAPS];
	if (md.diff) fr_pattern_diff(a, b); else fr_pattern(a, b);
	for (uint64_t w = 0; w < n_windows; w++) {
		const uint64_t first = w * FR_FRAME, end = std::min<uint64_t>(first + FR_FRAME, m - span);
		mdemod_frames_candidate best = { first, INT32_MIN, 0 };
		for (uint64_t p = first; p < end; p++)
			for (uint32_t H = 0; H < fr_mode_hyps(md); H++) {
				if (!fr_mode_allows(H, md)) continue;
				int32_t score = 0;
				for (int k = 0; k < FR_TAPS; k++) {
					int ip, qp;
					through(soft, m, p + FR_LEAD + k, H, ip, qp);
					score += ip * a[k] + qp * b[k];
				}
				if (md.diff && score < 0) score = -score;                      /* polarity is only a sign */
				if (score > best.score) { best.position = p; best.score = score; best.hypothesis = H; }   /* ascending p, H: the first of equals stays */
			}
		cand[w] = best;
	}
}

void
fr_model_frame(const int8_t *soft, uint64_t m, FrMode md, mdemod_frame_info &frame, uint8_t *cadu)
{
	uint8_t dbits[MDEMOD_FRAME_BYTES];
	for (int k = 0; k < 8; k++) model_sub_block(soft, m, frame, k, md.diff, cadu + k * (FR_SUB / 8), dbits + k * (FR_SUB / 8));
	frame.channel_errors = model_channel_errors(soft, m, frame, dbits);      /* counted on d, before the xor */
}

int
fr_settings(const mdemod_frames_opts *opts, mdemod_frames_opts &out)
{
	mdemod_frames_default_opts(&out);
	if (opts) out = *opts;
	if (out.min_run == 0) REFUSE("frames: min_run 0 (a run counts from 1 window or more)");
	if (out.piece_symbols == 0) out.piece_symbols = MDEMOD_FRAMES_DEFAULT_PIECE;
	if (out.piece_symbols % FR_FRAME || out.piece_symbols > (1ull << 30))
		REFUSE("frames: piece_symbols %llu must be a multiple of %u, at most 2^30", (unsigned long long)out.piece_symbols, FR_FRAME);
	return MDEMOD_OK;
}

int
fr_track(const mdemod_frames_opts &o, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m, std::vector<mdemod_frame_info> &frames)
{
	struct Run { uint64_t w1; uint32_t r, h, id; };
	std::vector<Run> counting;
	std::vector<mdemod_frame_info> all;
	uint32_t next_id = 0;
	auto emit = [&](uint64_t pos, int32_t score, uint32_t h, uint32_t flags, uint32_t id) {
		if (pos > m || m - pos < FR_FRAME) return;                           /* incomplete: it supported its run, it is not a frame */
		mdemod_frame_info f;
		memset(&f, 0, sizeof f);
		f.position = pos; f.score = score; f.hypothesis = h; f.flags = flags; f.run = id;
		all.push_back(f);
	};
	for (uint64_t w = 0; w < n_windows;) {
		const uint32_t r = static_cast<uint32_t>(cand[w].position % FR_FRAME), h = cand[w].hypothesis;
		uint64_t e = w + 1;
		while (e < n_windows && cand[e].position % FR_FRAME == r && cand[e].hypothesis == h) e++;
		if (e - w >= o.min_run) {
			uint32_t id = next_id;
			bool merged = false;
			for (size_t k = counting.size(); k-- > 0 && !merged;) {
				const Run &prev = counting[k];
				if (w - prev.w1 - 1 > o.flywheel) break;                     /* (the runs before it ended earlier still) */
				if (prev.r != r || prev.h != h) continue;
				id = prev.id;
				merged = true;
				for (uint64_t g = prev.w1 + 1; g < w; g++) emit(g * FR_FRAME + r, 0, h, MDEMOD_FRAME_FLYWHEEL, id);
			}
			if (!merged) next_id++;
			for (uint64_t g = w; g < e; g++) emit(cand[g].position, cand[g].score, h, 0, id);
			counting.push_back(Run{ e - 1, r, h, id });
		}
		w = e;
	}
	/* ascending, and no two overlap: a flywheel frame yields to a found one, else the earlier yields to the later */
	std::stable_sort(all.begin(), all.end(), [](const mdemod_frame_info &x, const mdemod_frame_info &y) { return x.position < y.position; });
	frames.clear();
	for (const mdemod_frame_info &f : all) {
		if (!frames.empty() && f.position - frames.back().position < FR_FRAME) {
			if ((f.flags & MDEMOD_FRAME_FLYWHEEL) && !(frames.back().flags & MDEMOD_FRAME_FLYWHEEL)) continue;
			frames.pop_back();
		}
		frames.push_back(f);
	}
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_frames_default_opts(mdemod_frames_opts *opts)
{
	if (!opts) return;
	opts->min_run = MDEMOD_FRAMES_DEFAULT_MIN_RUN;
	opts->flywheel = MDEMOD_FRAMES_DEFAULT_FLYWHEEL;
	opts->piece_symbols = 0;
}

uint64_t
mdemod_frames_windows(uint64_t m)
{
	return m > FR_SPAN ? (m - FR_SPAN + FR_FRAME - 1) / FR_FRAME : 0;
}

int
mdemod_frames_track(const mdemod_frames_opts *opts, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m,
                    mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames)
try { MDEMOD_API_ENTER
	if (!n_frames || (n_windows && !cand) || (cap && !frames)) REFUSE("mdemod_frames_track: the candidates, n_frames (and frames for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	const int rc = fr_settings(opts, o);
	if (rc) return rc;
	const int bad = fr_check_candidates(cand, n_windows, m, FrMode{ false, false });
	if (bad) return bad;
	std::vector<mdemod_frame_info> found;
	(void)fr_track(o, cand, n_windows, m, found);
	*n_frames = found.size();
	for (uint64_t i = 0; i < found.size() && i < cap; i++) frames[i] = found[i];
	return MDEMOD_OK;
} MDEMOD_API_CATCH

/* ------------------------------------------------------------------------------------------------------------ the model */

uint32_t
mdemod_frames_model_encode(const uint8_t *bytes, uint64_t n_bytes, uint32_t reg, int8_t *sym)
{
	reg &= 0x7Fu;
	for (uint64_t n = 0; n < 8 * n_bytes; n++) {
		reg = enc_step(reg, (bytes[n >> 3] >> (7 - (n & 7u))) & 1u);
		sym[2 * n] = static_cast<int8_t>(enc_c1(reg));
		sym[2 * n + 1] = static_cast<int8_t>(enc_c2(reg));
	}
	return reg;
}

void
mdemod_frames_model_pattern(int8_t *a, int8_t *b)
{
	fr_pattern(a, b);
}

int
mdemod_frames_model_candidates(const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand)
try { MDEMOD_API_ENTER
	const uint64_t n_windows = mdemod_frames_windows(m);
	if (n_windows && (!soft || !cand)) REFUSE("mdemod_frames_model_candidates: the symbols and the candidates are needed");
	int8_t a[FR_TAPS], b[FR_TAPS];
	fr_pattern(a, b);
	for (uint64_t w = 0; w < n_windows; w++) {
		const uint64_t first = w * FR_FRAME, end = std::min<uint64_t>(first + FR_FRAME, m - FR_SPAN);
		mdemod_frames_candidate best = { first, INT32_MIN, 0 };
		for (uint64_t p = first; p < end; p++) {
			int32_t A = 0, B = 0, Cc = 0, D = 0;
			const int8_t *x = soft + 2 * (p + FR_LEAD);
			for (int k = 0; k < FR_TAPS; k++) {
				const int32_t I = x[2 * k], Q = x[2 * k + 1];
				A += I * a[k]; B += Q * b[k]; Cc += I * b[k]; D += Q * a[k];
			}
			const int32_t score[8] = { A + B, Cc - D, -A - B, D - Cc, A - B, Cc + D, B - A, -Cc - D };
			for (uint32_t h = 0; h < 8; h++)
				if (score[h] > best.score) { best.position = p; best.score = score[h]; best.hypothesis = h; }   /* ascending p, h: the first of equals stays */
		}
		cand[w] = best;
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_frames_model_viterbi(const int8_t *soft, uint64_t m, mdemod_frame_info *frames, uint64_t n_frames, uint8_t *cadu)
try { MDEMOD_API_ENTER
	if (n_frames && (!soft || !frames || !cadu)) REFUSE("mdemod_frames_model_viterbi: the symbols, the frames and the output are needed");
	const int rc = fr_check_frames(frames, n_frames, m, FrMode{ false, false });
	if (rc) return rc;
	for (uint64_t f = 0; f < n_frames; f++) fr_model_frame(soft, m, FrMode{ false, false }, frames[f], cadu + f * MDEMOD_FRAME_BYTES);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_frames_model_decode(const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames,
                           uint64_t cap, uint64_t *n_frames)
try { MDEMOD_API_ENTER
	if (!n_frames || (m && !soft) || (cap && (!frames || !cadu))) REFUSE("mdemod_frames_model_decode: the symbols, n_frames (and the outputs for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	int rc = fr_settings(opts, o);
	if (rc) return rc;
	std::vector<mdemod_frames_candidate> cand(mdemod_frames_windows(m));
	rc = mdemod_frames_model_candidates(soft, m, cand.data());
	if (rc) return rc;
	std::vector<mdemod_frame_info> found;
	(void)fr_track(o, cand.data(), cand.size(), m, found);
	*n_frames = found.size();
	const uint64_t n = std::min<uint64_t>(found.size(), cap);
	rc = mdemod_frames_model_viterbi(soft, m, found.data(), n, cadu);
	if (rc) return rc;
	for (uint64_t i = 0; i < n; i++) frames[i] = found[i];
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
