/*
 * interleave_host.h — host side of the 80 k interleaved mode (include/meteor_demod_amd_interleave.h): the sync word's pattern, the
 * tracker (one copy: the product's and the model's) and the host model of the two kernels of csrc/interleave.hip.  HIP-free (the
 * CPU fuzz test builds csrc/interleave_host.cpp with gcc's sanitizers).
 */
#ifndef MDEMOD_INTERLEAVE_HOST_H
#define MDEMOD_INTERLEAVE_HOST_H

#include "../../include/meteor_demod_amd_interleave.h"

#define IL_BRANCHES  36u
#define IL_PERIOD    40u              /* symbols of a period: the sync word's 4 and 36 of data */
#define IL_SYNC      4u               /* symbols of the sync word = taps of the pattern */
#define IL_DATA_BITS 72u              /* bits of v in a period */
#define IL_WINDOW    2560u            /* positions of a window: 64 periods */
#define IL_HYPS      24u

#ifdef __cplusplus
#include <vector>

inline uint64_t il_windows(uint64_t m) { return m >= IL_SYNC ? (m - (IL_SYNC - 1) + IL_WINDOW - 1) / IL_WINDOW : 0; }

/* the sync word 0x27 as +-1: a[4] on I, b[4] on Q */
void il_pattern(int8_t a[IL_SYNC], int8_t b[IL_SYNC]);
/* opts (NULL = defaults) checked: MDEMOD_OK or MDEMOD_ERR_PARAM with the text noted */
int  il_settings(const mdemod_il_opts *opts, mdemod_il_opts &out);
/* every candidate in its window, at a phase below 40, with a hypothesis below 24; n_windows the count of m */
int  il_check_candidates(const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m);
/* a table the gather can take: MDEMOD_OK or MDEMOD_ERR_PARAM with the text noted */
int  il_check_segments(const mdemod_il_segment *segments, uint64_t n_segments, uint64_t n_periods, uint64_t m);
/* the tracker (arguments checked): the segments, and P */
void il_track(const mdemod_il_opts &o, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m, std::vector<mdemod_il_segment> &segments,
              uint64_t &n_periods);
/* the mean of the candidates' scores, rounded towards 0 (0 without a window) */
int32_t il_mean_score(const mdemod_frames_candidate *cand, uint64_t n_windows);

extern "C" {
#endif

/* ---- the host model: what the kernels of csrc/interleave.hip must compute, byte for byte (exported for the tests) ---- */

/* a[4], b[4] := the pattern */
void mdemod_il_model_pattern(int8_t *a, int8_t *b);
int  mdemod_il_model_candidates(const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand);
/* out[36 n_periods][2]; the arguments and the refusals of mdemod_il_deinterleave_device, everything in host memory */
int  mdemod_il_model_deinterleave(const mdemod_il_opts *opts, const int8_t *soft, uint64_t m, const mdemod_il_segment *segments, uint64_t n_segments,
                                  uint64_t n_periods, int8_t *out);

#ifdef __cplusplus
}
#endif
#endif
