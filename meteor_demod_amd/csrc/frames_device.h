/*
 * frames_device.h — what csrc/frames.hip offers the entries of the frame layer and of its link variant (csrc/frames_link.hip): the
 * kernels' launches and the two decoding pipelines, each under a mode (both switches off: the kernels of the plain layer).
 * Arguments are checked by the entries; the device is selected where the function takes one.
 */
#ifndef MDEMOD_FRAMES_DEVICE_H
#define MDEMOD_FRAMES_DEVICE_H

#include <hip/hip_runtime.h>

#include "frames_host.h"

/* one candidate per window of soft_dev[m] into cand_dev[fr_mode_windows(m, md)]; queued on st */
int fr_candidates_run(FrMode md, const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, hipStream_t st);
/* frames[0 .. n) of soft_dev[m] into cadu_dev; channel_errors into frames[].  Returns after the kernels have finished. */
int fr_viterbi_run(FrMode md, const int8_t *soft_dev, uint64_t m, mdemod_frame_info *frames, uint64_t n, uint8_t *cadu_dev, hipStream_t st);
/* search, tracker and decoding of a stream in device memory (*n_frames is 0 on entry; o comes from fr_settings) */
int fr_decode_device(FrMode md, const mdemod_frames_opts &o, const int8_t *soft_dev, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames, uint64_t cap,
                     uint64_t *n_frames, int device, hipStream_t st);
/* the same for a stream in host memory, copied in pieces of o.piece_symbols */
int fr_decode_host(FrMode md, const mdemod_frames_opts &o, const int8_t *soft, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames, uint64_t cap,
                   uint64_t *n_frames, int device);

#endif
