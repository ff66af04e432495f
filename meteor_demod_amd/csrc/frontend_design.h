/*
 * frontend_design.h — host side of the front end (include/meteor_demod_amd_frontend.h): the settings it accepts, its low-pass
 * filter and its phase steps.  HIP-free (the CPU fuzz test builds csrc/frontend_design.cpp with gcc's sanitizers).
 */
#ifndef MDEMOD_FRONTEND_DESIGN_H
#define MDEMOD_FRONTEND_DESIGN_H

#include <vector>
#include "../../include/meteor_demod_amd_frontend.h"

struct FeDesign {
	int32_t               decimation;      /* D                                          */
	int32_t               taps_per_phase;  /* (the default filled in)                    */
	uint32_t              n_taps;          /* L = taps_per_phase * D + 1, 1 for D = 1     */
	int32_t               samplerate_out;  /* fs / D                                     */
	std::vector<float>    taps;            /* h[0 .. L-1], symmetric, sum 1 (in double)  */
	std::vector<uint32_t> steps;           /* phase step per stream (n_streams entries)  */
};

/* The whole design: MDEMOD_OK, or MDEMOD_ERR_PARAM with mdm_note_error naming the setting.  n_streams = input.n_streams
 * (at least 1 step is produced). */
int mdemod_fe_design_host(const mdemod_params &input, const mdemod_fe_params &fe, FeDesign &out);
/* llround(-offset / fs * 2^32) mod 2^32 (offset already checked: finite, |offset| < fs / 2) */
uint32_t mdemod_fe_phase_step(double offset_hz, int32_t samplerate);

#endif
