/*
 * frames_host.h — host side of the frame layer (include/meteor_demod_amd_frames.h): the pattern, the tracker and the host model of
 * the kernels.  HIP-free (the CPU fuzz test builds csrc/frames_host.cpp with gcc's sanitizers).
 */
#ifndef MDEMOD_FRAMES_HOST_H
#define MDEMOD_FRAMES_HOST_H

#include "../../include/meteor_demod_amd_frames.h"

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

/* the pattern as +-1, from the encoder (the marker after 0xFF.. or 0x00..: the last 26 symbols are the same) */
void fr_pattern(int8_t a[FR_TAPS], int8_t b[FR_TAPS]);
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

#ifdef __cplusplus
}
#endif
#endif
