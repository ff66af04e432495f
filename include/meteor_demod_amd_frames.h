/*
 * meteor_demod_amd_frames.h — from soft symbols to CCSDS frames (CADUs, 1024 bytes each).
 *
 * The demodulator (include/meteor_demod_amd.h) ends in int8 soft symbols, as a `.s` file holds them.  The frame layer finds the
 * frames in such a stream (a correlation with the encoded sync marker at every symbol position, GPU), follows them (a tracker, host
 * code without GPU) and decodes them (Viterbi, GPU), and says for every frame how many channel bits the decoder corrected.
 * The entries below are QPSK framing.  Differential coding and a one-symbol skew between the rails (OQPSK at odd rotations: Meteor-M
 * N2-3 / N2-4) are the "link variant" specified at the end of this block; its entries are in include/meteor_demod_amd_frames_link.h.
 * The 80 k interleaved mode goes in front of this layer: include/meteor_demod_amd_interleave.h turns its raw symbols into a stream
 * these entries take.  Derandomising and Reed-Solomon follow in include/meteor_demod_amd_rs.h.
 * The specification of the kernels is a host model (csrc/frames_host.cpp, exported as mdemod_frames_model_*, csrc/frames_host.h):
 * everything is integer arithmetic, and GPU bytes equal model bytes.
 *
 *   input       int8 soft symbols soft[m][2] (I, Q).  All arithmetic on them is int32: negating -128 gives +128.
 *   code        rate 1/2, K = 7: reg = ((reg << 1) | bit) & 0x7F, c1 = parity(reg & 0x4F), c2 = parity(reg & 0x6D).  One info bit
 *               gives one symbol, c1 on I, c2 on Q; a coded 1 is a positive soft value.  The encoder runs on across frames and is
 *               never reset; bits are MSB first within a byte.  The marker 0x1ACFFC1D encoded from the zero state is
 *               0x035D49C24FF2686B (c1 first); its complement 0xFCA2B63DB00D9794 is the word LRPT decoders search for.
 *   frame       8192 symbols = 8192 info bits = 1024 bytes: the 4-byte marker and 1020 bytes.
 *   pattern     the first 6 symbols of an encoded marker depend on the bits before it, the last 26 do not: the pattern is those 26
 *               symbols, at offsets 6..31 from the frame start (the low 52 bits of the word above), as +-1: a[0..25] the c1 stream,
 *               b[0..25] the c2 stream.  It is derived from the encoder.
 *   hypotheses  h maps (I, Q) to (I', Q'):  0 (I, Q)  1 (-Q, I)  2 (-I, -Q)  3 (Q, -I)  4 (I, -Q)  5 (Q, I)  6 (-I, Q)  7 (-Q, -I):
 *               every sign and rail convention of the sender and of the Costas loop.
 *   scores      at position p, sums over k < 26 at symbol p + 6 + k: A = sum I a, B = sum Q b, C = sum I b, D = sum Q a; the scores
 *               of h = 0..7 are A+B, C-D, -A-B, D-C, A-B, C+D, B-A, -C-D.
 *   candidates  positions are p in [0, m - 32); window w covers the positions in [8192 w, 8192 (w + 1)).  A window's candidate is
 *               the (p, h, score) of its largest score; ties go to the lowest p, then the lowest h.  A window with no position has
 *               no candidate: there are ceil((m - 32) / 8192) windows (none for m <= 32).
 *   tracker     r = p mod 8192.  A run is a maximal chain of consecutive windows whose candidates share (r, h); it counts when it
 *               is at least min_run windows long.  Two counting runs with the same (r, h) are merged when the gap between them is
 *               at most `flywheel` windows (the later one joins the nearest earlier one): the frames of the gap are emitted at their
 *               predicted positions with MDEMOD_FRAME_FLYWHEEL (score 0).  A frame is emitted only if it is complete
 *               (p + 8192 <= m); the candidate of an incomplete last frame still counts towards its run.  A symbol slip or a
 *               rotation change starts a new run.  Frames come in ascending position and never overlap: where two would (a symbol
 *               deleted between two runs; a flywheel frame across another run), a flywheel frame yields to a found one, and
 *               otherwise the earlier frame yields to the later.
 *   decoding    a frame at p is decoded in 8 sub-blocks of 1024 info bits.  Sub-block k covers the symbols [s - 128, s + 1024 + 128)
 *               with s = p + 1024 k, clamped to [0, m), taken through hypothesis h.  The state is the last 6 input bits,
 *               s' = ((s << 1) | bit) & 63, with predecessors s' >> 1 and (s' >> 1) | 32.  Path metrics are int32, all 64 start at 0,
 *               not normalised (1280 steps x 254 fit); the branch metric I' o1 + Q' o2 (o: the branch's outputs as +-1) is
 *               maximised; on equal metrics the predecessor s' >> 1 wins.  Traceback starts from the largest final metric (ties:
 *               the lowest state); the bit of step t is the low bit of the state after step t; the middle 1024 bits are kept.
 *   report      per frame: position, hypothesis, score, flags, run, and channel_errors: the number of hard decisions (soft value
 *               through h > 0) that differ from the re-encoded decoded bits, over info bits 6..8191 of the frame (16372
 *               decisions), the encoder state taken from the frame's own first 6 decoded bits.
 *
 * The link variant (two switches, `differential` and `skew`; both off: everything above, byte for byte).  No off-air recording of
 * N2-3 / N2-4 was at hand: what binds is this text, a synthetic sender built to it and the OQPSK demodulator.
 *   differential  the sender's information bits b pass through NRZ-M before the encoder: d[t] = b[t] xor d[t-1]; the encoder sees d,
 *               the marker is coded like everything else.  Both generator masks have an odd number of taps, so
 *               encode(~d) = ~encode(d): polarity is only a sign.
 *   pattern     with `differential`: the 26 symbols at offsets 6..31 of the marker's 32 bits run through NRZ-M from d[-1] = 0 and
 *               encoded (derived from the encoder; d[-1] = 1 gives the complement).  The score of a position is |score| under this
 *               pattern, and only h in {0, 1, 4, 5} are reported: each 180 degree partner describes the same decoding.
 *   skew        the combined hypothesis is H = h + 8 s: s = 0 no skew; s = 1 symbol n is (I'[n], Q'[n+1]); s = 2 symbol n is
 *               (I'[n+1], Q'[n]), I' and Q' being the stream through h.  A rail value read at index m, one past the end, is 0.
 *               With `skew`, positions are p in [0, m - 33), there are ceil((m - 33) / 8192) windows, and all 24 H compete (the 12
 *               with h in {0, 1, 4, 5} with `differential`); ties go to the lowest p, then the lowest H.  Without `skew`:
 *               [0, m - 32) and H < 8, as above.
 *   tracker     unchanged, over (r, H): a skew change starts a new run as a rotation change does.
 *   decoding    as above with the symbols taken through H.  With `differential` the output bit of step t is d[t] xor d[t-1], with
 *               d[t-1] from the same sub-block's traceback (the 128-symbol lead-in supplies it; where the lead-in is clamped away,
 *               sub-block start 0, the bit before step 0 is 0).  Sub-blocks stay independent.  channel_errors is counted on d,
 *               before the xor, exactly as above.
 */
#ifndef METEOR_DEMOD_AMD_FRAMES_H
#define METEOR_DEMOD_AMD_FRAMES_H

#include "meteor_demod_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_FRAME_SYMBOLS        8192
#define MDEMOD_FRAME_BYTES          1024
#define MDEMOD_FRAME_DECISIONS      16372   /* what channel_errors is a count out of */
#define MDEMOD_FRAME_FLYWHEEL       1u      /* flags: no candidate stood here; the position is predicted from the runs around it */
#define MDEMOD_FRAMES_DEFAULT_MIN_RUN   3
#define MDEMOD_FRAMES_DEFAULT_FLYWHEEL  4
#define MDEMOD_FRAMES_DEFAULT_PIECE     (1ull << 26)

typedef struct {
	uint32_t min_run;             /* a run counts from this many windows (default 3; 0 is refused)                                */
	uint32_t flywheel;            /* counting runs of one (r, h) at most this many windows apart are merged (default 4; 0 = never)  */
	uint64_t piece_symbols;       /* mdemod_frames_decode_host copies pieces of this many symbols: 0 = 2^26, else a multiple of 8192 */
} mdemod_frames_opts;

typedef struct {
	uint64_t position;            /* the symbol at which the window's best score stands                                           */
	int32_t  score;
	uint32_t hypothesis;          /* 0..7                                                                                         */
} mdemod_frames_candidate;

typedef struct {
	uint64_t position;            /* first symbol of the frame                                                                    */
	int32_t  score;               /* the candidate's; 0 for a flywheel frame                                                      */
	uint32_t hypothesis;          /* 0..7; H = h + 8 s (below 24) from and to the link entries                                    */
	uint32_t flags;               /* MDEMOD_FRAME_FLYWHEEL                                                                        */
	uint32_t channel_errors;      /* of 16372; written by the decoding entries (0 from mdemod_frames_track)                        */
	uint32_t run;                 /* frames of one (merged) run share it: 0, 1, ... in the order the runs begin                   */
	uint32_t reserved;
} mdemod_frame_info;

/* The link variant's switches (include/meteor_demod_amd_frames_link.h).  All zero: the layer as the entries below compute it. */
typedef struct {
	uint32_t differential;        /* 1: NRZ-M coded sender (differential pattern, |score|, d[t] xor d[t-1] at traceback)                */
	uint32_t skew;                /* 1: the rails may stand one symbol apart: H = h + 8 s competes, s = 0, 1, 2                          */
	uint32_t reserved[2];         /* 0                                                                                                  */
} mdemod_frames_link;

/* min_run 3, flywheel 4, piece_symbols 0. */
void     mdemod_frames_default_opts(mdemod_frames_opts *opts);

/* Host only: the number of windows of a stream of m symbols (= candidates the entries below write). */
uint64_t mdemod_frames_windows(uint64_t m);

/* One candidate per window of soft_dev[m][2] (device memory), into cand_dev[mdemod_frames_windows(m)] (device memory).  Queued on
 * hip_stream of `device`; asynchronous.  m = 0 .. 32 is nothing to do, not an error.  Nothing outside soft_dev[0 .. m) is read. */
int  mdemod_frames_candidates_device(const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, int device, void *hip_stream);

/* Host only (no GPU): candidates (host memory, one per window of a stream of m symbols) give the frame list.  opts may be NULL
 * (defaults).  *n_frames := the number found; frames[0 .. min(cap, *n_frames)) are written; there are never more than m / 8192.
 * MDEMOD_ERR_PARAM (text in mdemod_last_error) for min_run 0, a candidate outside its window, a hypothesis above 7, n_windows
 * that is not mdemod_frames_windows(m). */
int  mdemod_frames_track(const mdemod_frames_opts *opts, const mdemod_frames_candidate *cand, uint64_t n_windows, uint64_t m,
                         mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames);

/* Decodes frames[0 .. n_frames) (host memory: position and hypothesis are read, channel_errors is written) of soft_dev[m][2] into
 * cadu_dev[n_frames][1024] (device memory).  Synchronous.  MDEMOD_ERR_PARAM for a frame that is not complete (position + 8192 > m)
 * or a hypothesis above 7. */
int  mdemod_frames_viterbi_device(const int8_t *soft_dev, uint64_t m, mdemod_frame_info *frames, uint64_t n_frames, uint8_t *cadu_dev,
                                  int device, void *hip_stream);

/* All three steps for a stream in device memory: cadu[min(cap, *n_frames)][1024] and frames[] in HOST memory.  Synchronous. */
int  mdemod_frames_decode_device(const mdemod_frames_opts *opts, const int8_t *soft_dev, uint64_t m, uint8_t *cadu,
                                 mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames, int device, void *hip_stream);

/* The same for a stream in host memory, copied in pieces: for the candidates a piece is opts->piece_symbols symbols from a multiple
 * of 8192 plus the correlator's 32; for the decoding it is the frames that begin within piece_symbols symbols, plus the 128 symbols
 * the sub-blocks need on each side.  The result is byte for byte that of mdemod_frames_decode_device on the whole stream. */
int  mdemod_frames_decode_host(const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m, uint8_t *cadu,
                               mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames, int device);

#ifdef __cplusplus
}
#endif
#endif
