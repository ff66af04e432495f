/*
 * meteor_demod_amd_frames_link.h — the link variant of the frame layer (include/meteor_demod_amd_frames.h): differential (NRZ-M)
 * coding and a one-symbol skew between the rails, what Meteor-M N2-3 / N2-4 (72 k OQPSK) need after `-m oqpsk`.  The specification
 * is the block "link variant" at the head of include/meteor_demod_amd_frames.h; the host model is mdemod_frames_model_link_*
 * (csrc/frames_host.h), and GPU bytes equal model bytes.  With both switches off (or link = NULL) every entry here is the entry of
 * the same name without `_link`, byte for byte; those keep refusing a hypothesis above 7.
 */
#ifndef METEOR_DEMOD_AMD_FRAMES_LINK_H
#define METEOR_DEMOD_AMD_FRAMES_LINK_H

#include "meteor_demod_amd_frames.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_FRAMES_SKEWS          3      /* s = 0, 1, 2: the combined hypothesis is H = h + 8 s, below 24 */

/* The window count of a stream of m symbols under `link`: ceil((m - 33) / 8192) with skew, mdemod_frames_windows(m) without. */
uint64_t mdemod_frames_link_windows(const mdemod_frames_link *link, uint64_t m);

/* mdemod_frames_candidates_device under `link`: cand_dev[mdemod_frames_link_windows(link, m)]; candidate.hypothesis carries H (with
 * `differential` only h in {0, 1, 4, 5}, and the score is the absolute value).  Nothing outside soft_dev[0 .. m) is read.  Queued on
 * hip_stream of `device`; asynchronous. */
int  mdemod_frames_link_candidates_device(const mdemod_frames_link *link, const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev,
                                          int device, void *hip_stream);

/* mdemod_frames_track over (r, H).  MDEMOD_ERR_PARAM as there, and for H of 24 or more (8 or more without `skew`), for a hypothesis
 * outside the differential set with `differential`, for n_windows that is not mdemod_frames_link_windows(link, m). */
int  mdemod_frames_link_track(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const mdemod_frames_candidate *cand,
                              uint64_t n_windows, uint64_t m, mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames);

/* mdemod_frames_viterbi_device with the symbols taken through frames[].hypothesis = H and, with `differential`, the NRZ-M undone
 * at traceback; channel_errors is counted on the decoder's own bits.  The same refusals for H as mdemod_frames_link_track.
 * Synchronous. */
int  mdemod_frames_link_viterbi_device(const mdemod_frames_link *link, const int8_t *soft_dev, uint64_t m, mdemod_frame_info *frames,
                                       uint64_t n_frames, uint8_t *cadu_dev, int device, void *hip_stream);

/* All three steps, as mdemod_frames_decode_device / mdemod_frames_decode_host.  The host entry's pieces are one symbol longer with
 * `skew` (the correlator's 33; the sub-blocks' 128 + 1 on the right); its result is byte for byte the device entry's.  Synchronous. */
int  mdemod_frames_link_decode_device(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const int8_t *soft_dev, uint64_t m,
                                      uint8_t *cadu, mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames, int device, void *hip_stream);
int  mdemod_frames_link_decode_host(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m,
                                    uint8_t *cadu, mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames, int device);

#ifdef __cplusplus
}
#endif
#endif
