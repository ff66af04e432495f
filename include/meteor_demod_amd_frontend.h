/*
 * meteor_demod_amd_frontend.h — digital down-converter (DDC) in front of the demodulator.
 *
 * The reference demodulates what it is given: a recording centred on the signal, at a rate it filters with a 2*order+1 tap RRC
 * whatever that rate is.  Most SDRs record far wider than LRPT (RTL-SDR 2.048 / 2.4 MS/s, Airspy 2.5 ... 10 MS/s, HackRF) and
 * often off-centre (tuned off the DC spike).  The front end moves a signal `offset_hz` from the recording's centre to 0 Hz,
 * low-pass filters it and keeps every D-th sample, on the GPU; the demodulator of include/meteor_demod_amd.h then runs on that
 * baseband (f32, fs / D) exactly as it runs on any f32 recording.
 *
 *   convert   u8 -> (int)b - 128, s16 as is, f32 as is (wavfile.c:58-69, as the demodulator kernels do)
 *   mix       z[n] = x[n] * e^{j theta(n)}, theta = 2 pi p(n) / 2^32, p(n) = n * step mod 2^32, step = llround(-offset / fs * 2^32)
 *             mod 2^32, n = absolute sample index since create / reset; e^{j theta} from two 1024-entry tables (20 bits of phase).
 *             step == 0 (offset 0): no mixer, the converted samples go through untouched
 *   filter    y[m] = sum_{k=0}^{L-1} h[k] z[m D - k], z[n < 0] = 0 (zero history, like the reference's Filter); L = taps_per_phase * D + 1
 *             (a Kaiser-windowed sinc, beta 8, cutoff fs / D / 2, sum h = 1), L = 1 and h = [1] for D = 1.  A call that brings a
 *             stream to N input samples has produced ceil(N / D) outputs in total.
 *
 * What is exact and what is not: the baseband is this library's own arithmetic (fixed summation order per output, explicit FMAs),
 * not the reference's; it is a pure function of the input values, the absolute index and the settings - how the input was cut
 * into calls, which batch slot the stream had and the run do not change a byte.  The demodulator on that baseband is the
 * reference's, bit for bit, as on any f32 input.
 */
#ifndef METEOR_DEMOD_AMD_FRONTEND_H
#define METEOR_DEMOD_AMD_FRONTEND_H

#include "meteor_demod_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_FE_MAX_DECIMATION   128
#define MDEMOD_FE_MIN_TAPS_PER_PHASE 8
#define MDEMOD_FE_MAX_TAPS_PER_PHASE 32
#define MDEMOD_FE_DEFAULT_TAPS_PER_PHASE 16
#define MDEMOD_FE_MAX_TAPS (MDEMOD_FE_MAX_TAPS_PER_PHASE * MDEMOD_FE_MAX_DECIMATION + 1)

typedef struct {
	double        offset_hz;        /* the signal's offset from the recording's centre (Hz, may be negative): moved to 0 Hz       */
	int32_t       decimation;       /* D, 1..128; fs must be a multiple of D, and fs / D >= 2.4 x symrate when D >= 2              */
	int32_t       taps_per_phase;   /* 8..32 (0 = the default, 16): L = taps_per_phase x D + 1                                    */
	const double *offsets_hz;       /* NULL, or one offset per stream (several channels of one recording): overrides offset_hz     */
} mdemod_fe_params;

typedef struct mdemod_fe mdemod_fe;

/* The filter and the phase step, on the host (no GPU): `input` describes the INPUT (samplerate, bps, symrate, n_streams for
 * offsets_hz).  taps may be NULL; otherwise cap >= L floats.  n_taps := L, step := the phase step of fe->offset_hz (of
 * offsets_hz[0] when given).  MDEMOD_ERR_PARAM, with mdemod_last_error() naming the setting, for: D or taps_per_phase out of
 * range, fs not a multiple of D, fs / D < 2.4 x symrate (D >= 2: the filter needs fs / D >= 3 x 0.8 symrate), an offset that is
 * not finite or not inside (-fs / 2, fs / 2). */
int  mdemod_fe_design(const mdemod_params *input, const mdemod_fe_params *fe, float *taps, uint32_t cap, uint32_t *n_taps,
                      uint32_t *step);

/* A front end for input->n_streams streams and the demodulator behind it: an ordinary mdemod_ctx with samplerate = fs / D and
 * bps = 32 (everything else, reserved flags included, is input's).  Refusals of that context's mdemod_create pass through. */
int  mdemod_fe_create(const mdemod_params *input, const mdemod_fe_params *fe, mdemod_fe **out);
void mdemod_fe_destroy(mdemod_fe *fe);
/* Every stream back to its power-on state: NCO index, filter history AND the inner demodulator (mdemod_reset).  Asynchronous
 * on hip_stream. */
int  mdemod_fe_reset(mdemod_fe *fe, void *hip_stream);
/* The inner demodulator (status, lock events, state, kernel name: include/meteor_demod_amd.h); owned by fe. */
mdemod_ctx *mdemod_fe_demodulator(mdemod_fe *fe);
/* Baseband outputs one call of n input samples produces at most: ceil(n / D). */
uint64_t mdemod_fe_max_outputs(const mdemod_fe *fe, uint64_t n_samples);

/* Front end only.  Ragged input as mdemod_process_device: stream s reads n_samples_dev[s] IQ samples from iq_dev +
 * iq_offset_dev[s] (device arrays, in samples, format of input->bps).  Stream s writes its outputs as interleaved f32 (I, Q) to
 * bb_dev + 2 * s * bb_stride and their count to n_out_dev[s] (device).  bb_cap <= bb_stride: outputs beyond bb_cap are dropped
 * (the state advances all the same; mdemod_fe_max_outputs of the largest count never is).  Asynchronous on hip_stream. */
int  mdemod_fe_baseband_device(mdemod_fe *fe, const void *iq_dev, const uint64_t *iq_offset_dev, const uint32_t *n_samples_dev,
                               float *bb_dev, uint64_t bb_stride, uint32_t bb_cap, uint32_t *n_out_dev, void *hip_stream);

/* Front end, then the ragged process call of the inner demodulator on its baseband; the per-stream counts go from the one to
 * the other in device memory, without a host sync.  max_samples: no count exceeds it (it sizes the baseband rows).  Soft
 * symbols as mdemod_process_device; status and lock events through mdemod_fe_demodulator(fe).  Asynchronous on hip_stream. */
int  mdemod_fe_process_device(mdemod_fe *fe, const void *iq_dev, const uint64_t *iq_offset_dev, const uint32_t *n_samples_dev,
                              uint32_t max_samples, int8_t *soft_dev, uint64_t soft_stride_symbols, uint32_t soft_cap_symbols,
                              void *hip_stream);

/* Host buffers, synchronous (as mdemod_process_host). */
int  mdemod_fe_process_host(mdemod_fe *fe, const void *const *iq_host, const uint32_t *n_samples,
                            int8_t *const *soft_host, const uint32_t *soft_cap, uint32_t *n_symbols);

/* ONE recording in host memory: the front end on the device, then mdemod_demodulate_recording on the baseband with
 * samplerate fs / D, bps 32 (input->n_streams and fe->offsets_hz are ignored).  Synchronous. */
int  mdemod_fe_demodulate_recording_host(const mdemod_params *input, const mdemod_fe_params *fe, const mdemod_recording_opts *opts,
                                         const void *iq_host, uint64_t n_samples, int8_t *soft_host, uint64_t soft_cap_symbols,
                                         mdemod_recording_report *report);

#ifdef __cplusplus
}
#endif
#endif
