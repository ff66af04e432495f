/*
 * frames_link_host.cpp — host side of the link variant of the frame layer (include/meteor_demod_amd_frames_link.h): the window
 * count, the tracker's entry over (r, H), and the host model's entries (mdemod_frames_model_link_*).  The arithmetic is that of
 * csrc/frames_host.cpp, taken under a mode; with both switches off every entry here hands on to the one without `_link`.  HIP-free.
 */
#include <algorithm>
#include <vector>

#include "frames_host.h"
#include "mdemod_internal_api.h"

extern "C" {

uint64_t
mdemod_frames_link_windows(const mdemod_frames_link *link, uint64_t m)
{
	return fr_mode_windows(m, FrMode{ false, link && link->skew });
}

int
mdemod_frames_link_track(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const mdemod_frames_candidate *cand, uint64_t n_windows,
                         uint64_t m, mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames)
try { MDEMOD_API_ENTER
	if (n_frames) *n_frames = 0;
	FrMode md;
	int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_track(opts, cand, n_windows, m, frames, cap, n_frames);
	if (!n_frames || (n_windows && !cand) || (cap && !frames)) REFUSE("mdemod_frames_link_track: the candidates, n_frames (and frames for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	if ((rc = fr_settings(opts, o)) || (rc = fr_check_candidates(cand, n_windows, m, md))) return rc;
	std::vector<mdemod_frame_info> found;
	(void)fr_track(o, cand, n_windows, m, found);
	*n_frames = found.size();
	for (uint64_t i = 0; i < found.size() && i < cap; i++) frames[i] = found[i];
	return MDEMOD_OK;
} MDEMOD_API_CATCH

/* ------------------------------------------------------------------------------------------------------------ the model */

void
mdemod_frames_model_link_pattern(const mdemod_frames_link *link, int8_t *a, int8_t *b)
{
	if (link && link->differential) fr_pattern_diff(a, b); else fr_pattern(a, b);
}

int
mdemod_frames_model_link_candidates(const mdemod_frames_link *link, const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand)
try { MDEMOD_API_ENTER
	FrMode md;
	const int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_model_candidates(soft, m, cand);
	if (fr_mode_windows(m, md) && (!soft || !cand)) REFUSE("mdemod_frames_model_link_candidates: the symbols and the candidates are needed");
	fr_model_candidates(soft, m, md, cand);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_frames_model_link_viterbi(const mdemod_frames_link *link, const int8_t *soft, uint64_t m, mdemod_frame_info *frames, uint64_t n_frames,
                                 uint8_t *cadu)
try { MDEMOD_API_ENTER
	FrMode md;
	int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_model_viterbi(soft, m, frames, n_frames, cadu);
	if (n_frames && (!soft || !frames || !cadu)) REFUSE("mdemod_frames_model_link_viterbi: the symbols, the frames and the output are needed");
	rc = fr_check_frames(frames, n_frames, m, md);
	if (rc) return rc;
	for (uint64_t f = 0; f < n_frames; f++) fr_model_frame(soft, m, md, frames[f], cadu + f * MDEMOD_FRAME_BYTES);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_frames_model_link_decode(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m, uint8_t *cadu,
                                mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames)
try { MDEMOD_API_ENTER
	if (n_frames) *n_frames = 0;
	FrMode md;
	int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_model_decode(opts, soft, m, cadu, frames, cap, n_frames);
	if (!n_frames || (m && !soft) || (cap && (!frames || !cadu))) REFUSE("mdemod_frames_model_link_decode: the symbols, n_frames (and the outputs for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	rc = fr_settings(opts, o);
	if (rc) return rc;
	std::vector<mdemod_frames_candidate> cand(fr_mode_windows(m, md));
	fr_model_candidates(soft, m, md, cand.data());
	std::vector<mdemod_frame_info> found;
	(void)fr_track(o, cand.data(), cand.size(), m, found);
	*n_frames = found.size();
	const uint64_t n = std::min<uint64_t>(found.size(), cap);
	for (uint64_t i = 0; i < n; i++) {
		fr_model_frame(soft, m, md, found[i], cadu + i * MDEMOD_FRAME_BYTES);
		frames[i] = found[i];
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
