/*
 * meteor_demod_amd_survey.h — where in a wide recording is the signal?
 *
 * The front end (include/meteor_demod_amd_frontend.h) moves a signal to 0 Hz if the caller knows its offset.  The survey finds
 * it: an averaged spectrum of the whole sampled band over the whole recording (GPU), a matched detector on that spectrum
 * (host), and a confirmation of every candidate by the estimators the recording stitcher uses (symbol-rate line and 4th-power
 * line, GPU), so that a carrier or an FM signal that is stronger than the LRPT signal is not taken for it.
 *
 *   spectrum  segments of fft_size samples side by side from sample 0 (no overlap; a trailing part shorter than a segment is
 *             not used); sample n of a segment is converted (u8 -> (int)b - 128, s16, f32 as is), multiplied by the periodic
 *             Hann window w[n] = 0.5 - 0.5 cos(2 pi n / fft_size) and transformed; |X|^2 is averaged.  The segments are split
 *             into n_rows runs of floor(segments / n_rows) segments (the last run takes the remainder): row r of
 *             psd[n_rows][fft_size] is the MEAN |X|^2 of its run, bin 0 = -fs / 2, frequency ascending.  No scaling besides.
 *             A row is a pure function of the samples and the settings: which block sums which segments, in which order, and
 *             the order in which the blocks' sums are added are fixed by (n_samples, fft_size, n_rows) alone; there are no
 *             float atomics.  Two runs give the same bytes.
 *   detect    noise floor = median of the rows' sum; circular correlation with the raised-cosine power shape of a signal of
 *             params->symrate (roll-off 0.6); the strongest peaks, each suppressing +-1.6 symrate around itself, interpolated
 *             over three points.
 *   confirm   every candidate through the front end (offset = the coarse one, all candidates in one call) on a window of the
 *             recording that starts in the candidate's strongest row, then mdemod_estimate_clock / mdemod_estimate_carrier on
 *             that baseband.  confirmed = clock_quality >= clock_threshold; the carrier estimate refines the offset only when
 *             carrier_quality >= carrier_threshold, else the coarse offset stands.
 */
#ifndef METEOR_DEMOD_AMD_SURVEY_H
#define METEOR_DEMOD_AMD_SURVEY_H

#include "meteor_demod_amd_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_SURVEY_MIN_FFT          256
#define MDEMOD_SURVEY_MAX_FFT          16384
#define MDEMOD_SURVEY_MAX_ROWS         4096
#define MDEMOD_SURVEY_MAX_CANDIDATES   32
#define MDEMOD_SURVEY_DEFAULT_CANDIDATES 8
#define MDEMOD_SURVEY_DEFAULT_ROWS     8
#define MDEMOD_SURVEY_DEFAULT_MIN_SNR_DB (-6.0)
#define MDEMOD_SURVEY_ROLLOFF          0.6     /* the reference's RRC_ALPHA (demod.h:8) */

typedef struct {
	uint32_t fft_size;            /* 0 = mdemod_survey_plan's; else a power of two, 256 .. 16384                                  */
	uint32_t n_rows;              /* rows of the waterfall the survey entries take (0 = 8); fewer when the recording is short     */
	uint32_t max_candidates;      /* 0 = 8; at most 32                                                                            */
	int32_t  decimation;          /* D of the confirmation's front end; 0 = the largest mdemod_fe_design accepts                  */
	double   min_snr_db;          /* candidates whose matched power over the floor is below this are dropped (default -6)         */
	float    clock_threshold;     /* confirmed = clock_quality >= this;    0 = MDEMOD_SURVEY_CLOCK_THRESHOLD                      */
	float    carrier_threshold;   /* offset refined when carrier_quality >= this; 0 = MDEMOD_SURVEY_CARRIER_THRESHOLD             */
} mdemod_survey_opts;

/* Each the geometric mean of the largest quality measured where there is no such line and the smallest where there is one
 * (profiles/survey.md: clock line 2.53 against 46.2, 4th-power line 3.56 against 24.1; the stitcher's own bar, recording.hip's
 * min_quality, is 8). */
#define MDEMOD_SURVEY_CLOCK_THRESHOLD   10.8f
#define MDEMOD_SURVEY_CARRIER_THRESHOLD 9.3f

typedef struct {
	double   offset_hz;           /* the refined offset when `refined`, else coarse_offset_hz                                     */
	double   coarse_offset_hz;    /* from the spectrum alone                                                                      */
	float    psd_snr_db;          /* matched power over the noise floor                                                           */
	float    clock_quality;       /* mdemod_estimate_clock's quality (0 from mdemod_survey_detect: not measured)                  */
	float    carrier_quality;     /* mdemod_estimate_carrier's quality (0 from mdemod_survey_detect)                              */
	uint32_t best_row;            /* the row in which the candidate's band is strongest                                           */
	int32_t  confirmed;           /* clock_quality >= clock_threshold                                                             */
	int32_t  refined;             /* offset_hz carries the carrier estimate                                                       */
} mdemod_survey_hit;

/* Everything to its default (fft_size 0, n_rows 8, max_candidates 8, decimation 0, min_snr_db -6, thresholds 0). */
void mdemod_survey_default_opts(mdemod_survey_opts *opts);

/* Host only.  fft_size := the smallest power of two with fs / fft_size <= symrate / 100, clamped to 256 .. 16384; decimation :=
 * the largest D in 1 .. 128 that divides fs with fs / D >= 2.4 x symrate.  Either pointer may be NULL.  MDEMOD_ERR_PARAM (text in
 * mdemod_last_error) for rates that are not positive, a format other than 8 / 16 / 32 bits, fs < 2.4 x symrate. */
int  mdemod_survey_plan(const mdemod_params *params, uint32_t *fft_size, int32_t *decimation);

/* The spectrum of one recording in device memory (format of params->bps; samplerate and the rest are not used): psd_dev
 * [n_rows][fft_size] f32.  MDEMOD_ERR_PARAM for an fft_size that is not a power of two in 256 .. 16384, n_rows outside
 * 1 .. 4096, a recording of fewer than n_rows segments.  Queued on hip_stream; the call returns after its kernels have
 * finished (its scratch memory lives for the call). */
int  mdemod_spectrum_device(const mdemod_params *params, const void *iq_dev, uint64_t n_samples, uint32_t fft_size, uint32_t n_rows,
                            float *psd_dev, void *hip_stream);

/* Host only (no GPU): candidates in a spectrum in host memory, strongest first.  opts may be NULL (defaults); of opts only
 * max_candidates and min_snr_db are used.  *n_hits := the number found; hits[0 .. min(cap, *n_hits)) are written, with
 * clock_quality, carrier_quality, confirmed and refined 0 and offset_hz = coarse_offset_hz.  Candidates closer to +-fs / 2 than
 * 0.8 symrate are dropped.  MDEMOD_ERR_PARAM for a setting out of range, a spectrum value that is not finite, fs < 2.4 x symrate
 * (nothing to survey). */
int  mdemod_survey_detect(const mdemod_params *params, const mdemod_survey_opts *opts, const float *psd, uint32_t fft_size,
                          uint32_t n_rows, mdemod_survey_hit *hits, uint32_t cap, uint32_t *n_hits);

/* Spectrum, detection, confirmation and refinement of one recording in device memory.  Hits come sorted: confirmed ones first,
 * then by psd_snr_db descending.  *n_hits := the number found; hits[0 .. min(cap, *n_hits)) are written.  Synchronous. */
int  mdemod_survey_device(const mdemod_params *params, const mdemod_survey_opts *opts, const void *iq_dev, uint64_t n_samples,
                          mdemod_survey_hit *hits, uint32_t cap, uint32_t *n_hits, void *hip_stream);

/* The same for a recording in host memory.  It is copied to the device in pieces of at most 2^28 samples; each piece
 * contributes whole rows to the waterfall (its share of n_rows by length), so the spectrum of a recording of several pieces is
 * NOT byte for byte that of mdemod_survey_device on the whole.  Synchronous. */
int  mdemod_survey_host(const mdemod_params *params, const mdemod_survey_opts *opts, const void *iq_host, uint64_t n_samples,
                        mdemod_survey_hit *hits, uint32_t cap, uint32_t *n_hits);

#ifdef __cplusplus
}
#endif
#endif
