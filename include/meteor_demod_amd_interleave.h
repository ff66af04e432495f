/*
 * meteor_demod_amd_interleave.h — the 80 k interleaved mode: from the raw soft symbols of such a link to the soft-symbol stream the
 * frame layer (include/meteor_demod_amd_frames.h, plain or `differential`) decodes unchanged.
 *
 * The layer finds the interleaver's sync word under every sign, rail and skew convention (GPU), follows it across symbol slips and
 * rotation changes (a tracker, host code without GPU), and then strips the sync words, resolves the convention and deinterleaves in
 * one gather (GPU).  The specification of the kernels is a host model (csrc/interleave_host.cpp, exported as mdemod_il_model_*):
 * everything is integer arithmetic, and GPU bytes equal model bytes.  No off-air 80 k recording was at hand: what binds is this
 * text and a synthetic sender built to it.  The first recording confirms (or corrects) the bit order within a symbol and the
 * direction of the branch delays.  h, s, H = h + 8 s, "the stream through H" and "a rail value read at index m is 0" are those of
 * include/meteor_demod_amd_frames.h.
 *
 *   bit stream    the coded symbols (c1, c2) of the K = 7 encoder as bits u[2n] = c1, u[2n + 1] = c2; a coded 1 is a positive value.
 *   interleaver   36 branches, branch delay M (`branch_delay`, default 2048).  Bit k is on branch k mod 36 and leaves 36 M (k mod 36)
 *                 bit times late: v[k] = u[k - 36 M (k mod 36)]; a negative index is whatever the sender's registers held.
 *   sync word     before every 72 bits of v stand the 8 bits of 0x27, MSB first.  Period N of the channel stream c is
 *                 c[80 N .. 80 N + 7] = sync word, c[80 N + 8 + j] = v[72 N + j], j < 72.  Channel symbol i is (c[2 i], c[2 i + 1])
 *                 on (I, Q): a period is 40 symbols, the sync word 4 - the four constellation points, so it resolves all 24 H by
 *                 itself.  72 = 2 x 36: the bit after a sync word is always on branch 0.  As +-1 the sync word is
 *                 a = (-1, +1, -1, +1) on I and b = (-1, -1, +1, +1) on Q.
 *   sync search   a position p is a symbol index with p + 4 <= m; score(p, H) = sum over i < 4 of a[i] I"[p + i] + b[i] Q"[p + i],
 *                 (I", Q") the stream through H, in int32.  Window w covers the positions in [2560 w, 2560 (w + 1)): 64 periods;
 *                 there are ceil((m - 3) / 2560) windows (none for m < 4).  In a window, phase r < 40 scores the sum of score(p, H)
 *                 over the window's positions p = r (mod 40); only phases that have a position compete, and all 24 H.  The window's
 *                 candidate is the (r, H) of the largest sum; ties go to the lowest r, then the lowest H.  It is reported as a
 *                 mdemod_frames_candidate: position = 2560 w + r, hypothesis = H, score = the sum (|score| <= 64 x 8 x 128).
 *   tracker       a run is a maximal chain of consecutive windows whose candidates share (r, H); it counts from min_run windows.
 *                 The counting runs, in order, give the segments; a counting run with the (r, H) of the current segment continues
 *                 it.  Segment 0 begins at symbol 0, every later one at the first symbol of its run's first window; a segment ends
 *                 where the next begins, the last at m (windows in no counting run belong to the segment before them).  Per
 *                 segment: x0, the smallest x >= its first symbol with x = r (mod 40), and the period index N0: 0 for segment 0,
 *                 N0[i + 1] = N0[i] + floor((x0[i + 1] - x0[i] + 20) / 40) - a slip of fewer than 20 symbols keeps the sender's
 *                 count.  P, the number of periods, is N0_last + floor((m - x0_last) / 40); no counting run: no segment and P = 0,
 *                 which is a result, not an error.  A slip is located to one window, not finer.
 *   gather        the output is int8 out[36 P][2], bit k < 72 P at byte k: k' = k + 36 M (k mod 36), N = k' div 72, j = k' mod 72.
 *                 N >= P: 0.  Otherwise, with i the last segment with N0[i] <= N and x = x0[i] + 40 (N - N0[i]) + 4 + j div 2, the
 *                 bit is rail j mod 2 of symbol x through H[i] (skew reads that rail at x or x + 1 as H says; an index >= m reads
 *                 0; a negated -128 is stored as +127).  Out bit k is the sender's u[k] in the sender's own convention (h = 0,
 *                 s = 0): a stream the frame layer takes with `skew` off.  The last 35 x 36 M bits are partly zeros (erasures):
 *                 the interleaver's latency, not a defect.
 */
#ifndef METEOR_DEMOD_AMD_INTERLEAVE_H
#define METEOR_DEMOD_AMD_INTERLEAVE_H

#include "meteor_demod_amd_frames.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_IL_BRANCHES              36
#define MDEMOD_IL_PERIOD_SYMBOLS        40      /* 4 of the sync word, 36 of data */
#define MDEMOD_IL_WINDOW_SYMBOLS        2560    /* 64 periods */
#define MDEMOD_IL_HYPOTHESES            24
#define MDEMOD_IL_DEFAULT_BRANCH_DELAY  2048
#define MDEMOD_IL_DEFAULT_MIN_RUN       3

typedef struct {
	uint32_t branch_delay;        /* M (default 2048; 0 is refused)                                                               */
	uint32_t min_run;             /* a run counts from this many windows (default 3; 0 is refused)                                */
	uint32_t reserved[2];         /* 0                                                                                            */
} mdemod_il_opts;

typedef struct {
	uint64_t first_symbol;        /* the segment begins here: 0, or the first symbol of a window                                  */
	uint64_t marker_symbol;       /* x0: the first sync word of the segment stands here                                           */
	uint64_t period;              /* N0: the sender's period index at x0                                                          */
	uint32_t phase;               /* r = x0 mod 40                                                                                */
	uint32_t hypothesis;          /* H = h + 8 s, below 24                                                                        */
} mdemod_il_segment;

/* branch_delay 2048, min_run 3. */
void     mdemod_il_default_opts(mdemod_il_opts *opts);

/* Host only: the number of windows of a stream of m symbols, and the symbols an output buffer for such a stream has room for:
 * 36 floor(m / 40) + 36. */
uint64_t mdemod_il_windows(uint64_t m);
uint64_t mdemod_il_max_output_symbols(uint64_t m);

/* One candidate per window of soft_dev[m][2] (device memory, any 2-byte alignment) into cand_dev[mdemod_il_windows(m)] (device
 * memory).  Queued on hip_stream of `device`; asynchronous.  m < 4 is nothing to do.  Nothing outside soft_dev[0 .. m) is read. */
int  mdemod_il_candidates_device(const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, int device, void *hip_stream);

/* Host only (no GPU): candidates (host memory) give the segment list.  opts may be NULL (defaults).  *n_segments := the number
 * found, segments[0 .. min(cap, *n_segments)) are written, *n_periods := P.  MDEMOD_ERR_PARAM (text in mdemod_last_error) for
 * min_run 0, branch_delay 0, a candidate outside its window (or at a phase of 40 and more), a hypothesis of 24 and more, n_windows
 * that is not mdemod_il_windows(m). */
int  mdemod_il_track(const mdemod_il_opts *opts, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m,
                     mdemod_il_segment *segments, uint64_t cap, uint64_t *n_segments, uint64_t *n_periods);

/* The gather: soft_dev[m][2] through segments[0 .. n_segments) (HOST memory: marker_symbol, period and hypothesis are read) into
 * out_dev[36 n_periods][2] (device memory).  The input and the output ranges must be apart.  Queued on hip_stream; asynchronous
 * for up to 32 segments (they travel as kernel arguments), synchronous for more.  MDEMOD_ERR_PARAM for a table that does not
 * begin at period 0 or whose periods descend, a hypothesis of 24 and more, a marker_symbol above m, n_periods above m. */
int  mdemod_il_deinterleave_device(const mdemod_il_opts *opts, const int8_t *soft_dev, uint64_t m, const mdemod_il_segment *segments,
                                   uint64_t n_segments, uint64_t n_periods, int8_t *out_dev, int device, void *hip_stream);

/* All three steps for a stream in device memory.  out_dev[out_cap][2] (device memory; mdemod_il_max_output_symbols(m) symbols hold
 * every stream but one with a slip in nearly every window) receives the first min(36 P, out_cap rounded down to a multiple of 36)
 * symbols of the gather; segments[0 .. min(cap, *n_segments)) in HOST memory; *n_periods := P.  *mean_score (may be NULL) := the mean
 * of the candidates' scores: 64 x 8 x the signal's amplitude on a clean link.  Synchronous. */
int  mdemod_il_decode_device(const mdemod_il_opts *opts, const int8_t *soft_dev, uint64_t m, int8_t *out_dev, uint64_t out_cap,
                             mdemod_il_segment *segments, uint64_t cap, uint64_t *n_segments, uint64_t *n_periods, int32_t *mean_score,
                             int device, void *hip_stream);

/* The same for a stream and an output in host memory.  The whole stream is uploaded at once: a 15-minute pass is 144 MB, and the
 * gather reaches 35 x 36 x 2048 bits = 1.29 M symbols ahead, which makes pieces pointless. */
int  mdemod_il_decode_host(const mdemod_il_opts *opts, const int8_t *soft, uint64_t m, int8_t *out, uint64_t out_cap,
                           mdemod_il_segment *segments, uint64_t cap, uint64_t *n_segments, uint64_t *n_periods, int32_t *mean_score,
                           int device);

#ifdef __cplusplus
}
#endif
#endif
