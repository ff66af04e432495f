/*
 * survey_detect.h — host side of the survey (include/meteor_demod_amd_survey.h): its settings, the plan and the detector on a
 * spectrum.  HIP-free (the CPU fuzz test builds csrc/survey_detect.cpp with gcc's sanitizers).
 */
#ifndef MDEMOD_SURVEY_DETECT_H
#define MDEMOD_SURVEY_DETECT_H

#include <vector>
#include "../../include/meteor_demod_amd_survey.h"

struct SurveySettings {
	uint32_t fft_size, n_rows, max_candidates;
	int32_t  decimation;
	double   min_snr_db;
	float    clock_threshold, carrier_threshold;
};

/* opts (NULL = defaults) with every default filled in and every setting checked: MDEMOD_OK, or MDEMOD_ERR_PARAM with
 * mdm_note_error naming the setting.  fft_size and decimation come from the plan where opts leaves them 0. */
int mdemod_survey_settings(const mdemod_params &params, const mdemod_survey_opts *opts, SurveySettings &out);
/* fft_size a power of two in 256 .. 16384 */
bool mdemod_survey_fft_size_ok(uint32_t fft_size);
/* the detector proper (settings already checked): hits strongest first */
int mdemod_survey_detect_host(const mdemod_params &params, const SurveySettings &s, const float *psd, uint32_t fft_size, uint32_t n_rows,
                              std::vector<mdemod_survey_hit> &hits);

#endif
