/*
 * frames_host.h — host side of the frame layer (include/meteor_demod_amd_frames.h): the pattern, the tracker and the host model of
 * the kernels.  HIP-free (the CPU fuzz test builds csrc/frames_host.cpp with gcc's sanitizers).
 */
#ifndef MDEMOD_FRAMES_HOST_H
#define MDEMOD_FRAMES_HOST_H

#include "../../include/meteor_demod_amd_frames.h"
#include "../../include/meteor_demod_amd_frames_link.h"

#define FR_FRAME     8192u            /* symbols = info bits of a frame */
#define FR_TAPS      26               /* the pattern: symbols 6..31 of an encoded marker */
#define FR_LEAD      6
#define FR_SPAN      32               /* FR_LEAD + FR_TAPS: a position needs this many symbols */
#define FR_SUB       1024             /* info bits a sub-block keeps */
#define FR_HALO      128              /* symbols decoded and dropped on each side of them */
#define FR_STEPS     (FR_SUB + 2 * FR_HALO)

#ifdef __cplusplus
#include <vector>

/* how hypothesis h reads (I, Q): I' = si * (swap ? Q : I), Q' = sq * (swap ? I : Q) */
struct FrHyp { int si, sq, swap; };
inline FrHyp
fr_hyp(uint32_t h)
{
	static const FrHyp T[8] = { { 1, 1, 0 }, { -1, 1, 1 }, { -1, -1, 0 }, { 1, -1, 1 }, { 1, -1, 0 }, { 1, 1, 1 }, { -1, 1, 0 }, { -1, -1, 1 } };
	return T[h & 7];
}

/* the link variant (include/meteor_demod_amd_frames_link.h): the two switches, and what follows from them.  H = h + 8 s. */
struct FrMode { bool diff, skew; };
inline bool fr_mode_plain(FrMode md) { return !md.diff && !md.skew; }
inline uint32_t fr_mode_span(FrMode md) { return FR_SPAN + (md.skew ? 1u : 0u); }            /* a position and its skewed sums need this many symbols */
inline uint64_t fr_mode_windows(uint64_t m, FrMode md) { return m > fr_mode_span(md) ? (m - fr_mode_span(md) + FR_FRAME - 1) / FR_FRAME : 0; }
inline uint32_t fr_mode_hyps(FrMode md) { return md.skew ? 24u : 8u; }
inline bool fr_mode_allows(uint32_t H, FrMode md) { return H < fr_mode_hyps(md) && !(md.diff && (H & 2u)); }   /* differential: h in {0, 1, 4, 5} */
/* link (NULL = both off) checked: MDEMOD_OK or MDEMOD_ERR_PARAM with the text noted */
int  fr_mode_of(const mdemod_frames_link *link, FrMode &md);

/* the pattern as +-1, from the encoder (the marker after 0xFF.. or 0x00..: the last 26 symbols are the same) */
void fr_pattern(int8_t a[FR_TAPS], int8_t b[FR_TAPS]);
/* the differential pattern: the marker through NRZ-M from d[-1] = 0, encoded (d[-1] = 1 gives the complement) */
void fr_pattern_diff(int8_t a[FR_TAPS], int8_t b[FR_TAPS]);
/* every frame complete and its hypothesis one the mode allows: MDEMOD_OK or MDEMOD_ERR_PARAM with the text noted */
int  fr_check_frames(const mdemod_frame_info *frames, uint64_t n_frames, uint64_t m, FrMode md);
/* every candidate in its window and its hypothesis one the mode allows */
int  fr_check_candidates(const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m, FrMode md);
/* the model's pieces under a mode (arguments checked; both switches off: what mdemod_frames_model_* compute) */
void fr_model_candidates(const int8_t *soft, uint64_t m, FrMode md, mdemod_frames_candidate *cand);
void fr_model_frame(const int8_t *soft, uint64_t m, FrMode md, mdemod_frame_info &frame, uint8_t *cadu);
/* opts (NULL = defaults) checked: MDEMOD_OK or MDEMOD_ERR_PARAM with the text noted; piece_symbols 0 becomes 2^26 */
int  fr_settings(const mdemod_frames_opts *opts, mdemod_frames_opts &out);
/* the tracker (arguments checked) */
int  fr_track(const mdemod_frames_opts &o, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m, std::vector<mdemod_frame_info> &frames);

extern "C" {
#endif

/* ---- the host model: what the kernels of csrc/frames.hip must compute, byte for byte (exported for the tests) ---- */

/* n_bytes bytes, MSB first, through the encoder from register `reg`: sym[8 n_bytes][2] := (c1, c2) as +-1.  Returns the register after. */
uint32_t mdemod_frames_model_encode(const uint8_t *bytes, uint64_t n_bytes, uint32_t reg, int8_t *sym);
/* a[26], b[26] := the pattern */
void mdemod_frames_model_pattern(int8_t *a, int8_t *b);
int  mdemod_frames_model_candidates(const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand);
int  mdemod_frames_model_viterbi(const int8_t *soft, uint64_t m, mdemod_frame_info *frames, uint64_t n_frames, uint8_t *cadu);
int  mdemod_frames_model_decode(const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames,
                                uint64_t cap, uint64_t *n_frames);

/* ---- the model of the link variant (csrc/frames_link_host.cpp; link = NULL or both switches off: the entries above) ---- */

/* a[26], b[26] := the pattern the candidates of `link` correlate with (the differential one with `differential`) */
void mdemod_frames_model_link_pattern(const mdemod_frames_link *link, int8_t *a, int8_t *b);
int  mdemod_frames_model_link_candidates(const mdemod_frames_link *link, const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand);
int  mdemod_frames_model_link_viterbi(const mdemod_frames_link *link, const int8_t *soft, uint64_t m, mdemod_frame_info *frames, uint64_t n_frames,
                                      uint8_t *cadu);
int  mdemod_frames_model_link_decode(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m, uint8_t *cadu,
                                     mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames);

#ifdef __cplusplus
}
#endif
#endif
