/*
 * meteor_demod_amd_image.h — from transfer frames (VCDUs, include/meteor_demod_amd_rs.h) to pictures: the M-PDU packet zone
 * demultiplexed into CCSDS space packets, and the MSU-MR image packets decoded into strips of 8 x 112 pixels (GPU), which the host
 * places into one picture per channel.  The specification of the two kernels is a host model in integer arithmetic
 * (csrc/image_host.cpp, exported as mdemod_image_model_*): GPU bytes equal model bytes.  The signal behind the tests is a synthetic
 * sender (mdemod_image_model_encode_packet); see "to be confirmed off air" at the end.
 *
 *   VCDU        892 bytes.  0 .. 5 the primary header (mdemod_rs_vcdu_header), 6 .. 7 the insert zone, 8 .. 9 the M-PDU header with
 *               the first-header pointer fhp = ((b8 & 7) << 8) | b9 (the five upper bits of b8 are spare and not looked at),
 *               10 .. 891 the packet zone of 882 bytes.  fhp = 0x7FF: no packet starts in this frame.  Any other value above 881 is
 *               invalid.  The payload stream of a batch of n frames has byte p at vcdu[p / 882][10 + p % 882], p < 882 n.
 *   usable      a frame is usable when its version is 1, its vcid is opts.vcid, its mdemod_rs_info (when an array is given) is
 *               not MDEMOD_RS_UNCORRECTABLE and its fhp is not invalid.  Frames f and f + 1 are linked when both are usable and
 *               counter(f + 1) == (counter(f) + 1) mod 2^24.
 *   packet      a 6-byte primary header h0 .. h5: apid = ((h0 & 7) << 8) | h1, secondary-header flag (h0 >> 3) & 1, sequence
 *               flags h2 >> 6, seq = ((h2 & 0x3f) << 8) | h3, total length 7 + ((h4 << 8) | h5) (7 .. 65 542).
 *   demux       the walk of usable frame f with fhp(f) != 0x7FF starts at pos = fhp(f).  While pos < 882: the header is read at
 *               stream position s = 882 f + pos (its bytes may lie in frame f + 1), end = s + length, g = end / 882, e = end % 882,
 *               and the packet is accepted if and only if
 *                 - every frame from f to the frame of its last byte, (end - 1) / 882, and to the frame of the header's last byte,
 *                   (s + 5) / 882, lies inside the batch and each is linked to the one before it;
 *                 - every frame strictly between f and g has fhp = 0x7FF;
 *                 - when g > f and e > 0: fhp(g) == e;
 *                 - when e == 0 (the packet ends on a frame's end) and frame g is inside the batch and linked to g - 1: fhp(g) == 0.
 *               An accepted packet gives a descriptor and pos += length.  A packet that is not accepted ends the walk of its frame.
 *               Descriptors are listed in stream order (by frame, then by position); idle packets (apid 2047) are included.  A
 *               frame yields at most 126 descriptors.
 *   descriptor  mdemod_packet, 16 bytes: start (stream position of the header), length (total), apid, seq, flags = sequence flags
 *               | secondary-header flag << 2.
 *
 *   image       a descriptor is an image packet when apid is 64 .. 69, the secondary-header flag is set and length >= 21.  The
 *               decoder takes apid, flag and length from the descriptor and every byte behind the 6 header bytes from the stream:
 *               6 .. 7 day (big endian, as all fields), 8 .. 11 ms of day, 12 .. 13 us, 14 mcun, 15 .. 16 scan header, 17 .. 18
 *               segment header (0xFFF0), 19 q, 20 .. length - 1 the bit stream.
 *   bit stream  MSB first, no byte stuffing, no restart markers.  14 blocks.  Per block: one DC code (category s = 0 .. 11, then s
 *               extra bits, EXTEND of JPEG F.2.2.1: v < 2^(s-1) ? v - 2^s + 1 : v) added to the predictor (0 at the start of every
 *               packet); then AC codes from k = 1: symbol 0x00 ends the block, 0xF0 skips 16 (k += 16; the block fails if k > 64),
 *               any other symbol (r << 4) | s: k += r, the block fails if k > 63, s extra bits (EXTEND) are coefficient k in zigzag
 *               order, k += 1; the block is complete at k = 64 too.  A code is matched bit by bit, at most 16 bits.
 *   DC table    BITS 00 01 05 01 01 01 01 01 01 00 00 00 00 00 00 00, values 00 01 02 03 04 05 06 07 08 09 0a 0b  (JPEG K.3)
 *   AC table    BITS 00 02 01 03 03 02 04 03 05 05 04 04 00 00 01 7d, values                                      (JPEG K.5)
 *               01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 82 09
 *               0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65
 *               66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9
 *               aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea
 *               f1 f2 f3 f4 f5 f6 f7 f8 f9 fa
 *               Codes are canonical (JPEG Annex C): within a length in the order of the values, the first code of a length is
 *               (last code of the length before + 1) << 1.
 *   zigzag      k -> 8 row + column:  0  1  8 16  9  2  3 10 17 24 32 25 18 11  4  5 12 19 26 33 40 48 41 34 27 20 13  6  7 14 21 28
 *                                    35 42 49 56 57 50 43 36 29 22 15 23 30 37 44 51 58 59 52 45 38 31 39 46 53 60 61 54 47 55 62 63
 *   quantiser   std (JPEG K.1, by 8 row + column):  16 11 10 16 24 40 51 61 / 12 12 14 19 26 58 60 55 / 14 13 16 24 40 57 69 56 /
 *               14 17 22 29 51 87 80 62 / 18 22 37 56 68 109 103 77 / 24 35 55 64 81 104 113 92 / 49 64 78 87 103 121 120 101 /
 *               72 92 95 98 112 100 103 99.  For 20 < q < 50: qt[i] = max(1, (5000 std[i] + 50 q) / (100 q)); otherwise, with
 *               F = 200 - 2 q: qt[i] = F <= 0 ? 1 : max(1, (F std[i] + 50) / 100).  Integer division: round(std f / 100), halves up,
 *               f = 5000 / q or F.  Coefficient k of the stream times qt[zigzag[k]], saturated to -2048 .. 2047, is in[zigzag[k]].
 *   inverse DCT 32-bit integers throughout; >> is the arithmetic shift (floor).  N[0 .. 8] = 131072 181802 171254 154124 131072
 *               102983 70936 36163 0 (round(2^17 sqrt 2 cos(j pi / 16)); N[0] is not used).  With c(j) for j = 0 .. 31: N[j] for
 *               j <= 8, -N[16 - j] for 8 < j <= 16, c(32 - j) above: M[x][0] = 131072 and M[x][u] = c((2 x + 1) u mod 32), u = 1 .. 7.
 *               Pass 1, columns: t[8 y + u] = (sum over v of M[y][v] in[8 v + u] + 2048) >> 12.
 *               Pass 2, rows: hi = t >> 9, lo = t & 511; A = sum over u of M[x][u] hi[8 y + u], B = the same over lo;
 *               R = A + ((B + 256) >> 9); pixel[8 y + x] = clamp(128 + ((R + 32768) >> 16), 0, 255).
 *               (The transform is the textbook one with 1 / (2 sqrt 2) taken out of both passes: DC alone gives exactly
 *               floor(DC / 8 + 1 / 2).  No sum passes 2^31: |in| <= 2048, a row of |M| sums to less than 7.4724 * 2^17.  Its error
 *               against the real-valued transform stays below 0.2 grey levels for every input.)
 *   failure     a block fails when the bit stream runs past the packet's last byte, when 16 bits match no code, or when a
 *               coefficient index passes 63 (above).  Blocks before it keep their pixels; it and all later blocks are zero.
 *               mcus says how many were decoded (0 .. 14) and bits_used where the last decoded block ended.
 *   strip       uint8 [8][112], block k in columns 8 k .. 8 k + 7.
 *   report      mdemod_strip_info, 16 bytes.  Flags: NOT_IMAGE (apid, flag or length outside the rule: strip and report zero but
 *               for the flag), BAD_HEADER (mcun not a multiple of 14 or above 182, or the segment header not 0xFFF0; the strip is
 *               still decoded), TRUNCATED (mcus < 14), OUTSIDE (the descriptor's length is outside 7 .. 65 542 or it points beyond
 *               the batch: nothing is read, strip and report zero but for the flag).
 *
 *   placement   (host) apids[3], default 64 65 66: slot k is the index in it.  period, default 43: 3 x 14 image packets and one
 *               packet of apid 70 per strip of 8 lines, the 14-bit sequence count running across the apids.  Candidates are the
 *               descriptors of an active apid whose report has none of NOT_IMAGE, BAD_HEADER, OUTSIDE, in list order.  The anchor
 *               is the first candidate without any flag: first = seq - 14 k - mcun / 14.  Candidates before the anchor are dropped
 *               (they would land before row 0).  From the anchor on a seq below the previous candidate's adds 16 384 to all that
 *               follow; with seq' the sum, the strip row is (seq' - first) / period, the cell mcun / 14: the strip lands at line
 *               8 row, column 8 mcun of its channel's picture.  A row above 65 535 is dropped.  The width is 1568, the height 8 x
 *               (the largest row + 1), cells never filled are 0, and filled[height / 8][14] per channel says which are.
 *
 *   to be confirmed off air   there is no off-air recording behind any of this yet.  The first one confirms: the counting
 *               convention (one sequence counter across the apids, period 43), the active apid set, and the rounding of the
 *               quantiser (halves up, and the two branches at q = 20 and q = 50).
 */
#ifndef METEOR_DEMOD_AMD_IMAGE_H
#define METEOR_DEMOD_AMD_IMAGE_H

#include "meteor_demod_amd_rs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_IMAGE_ZONE_BYTES      882
#define MDEMOD_IMAGE_NO_HEADER       0x7FFu
#define MDEMOD_IMAGE_MAX_PER_FRAME   126      /* descriptors one frame can yield: cap = 126 n always suffices */
#define MDEMOD_IMAGE_MCUS            14
#define MDEMOD_IMAGE_STRIP_BYTES     (8 * 112)
#define MDEMOD_IMAGE_WIDTH           1568
#define MDEMOD_IMAGE_CELLS           14       /* strips side by side in a picture */
#define MDEMOD_IMAGE_MAX_ROWS        65536
#define MDEMOD_IMAGE_OVERLAP         76       /* frames a packet that starts in one frame can reach into, and the one after */

#define MDEMOD_STRIP_NOT_IMAGE       1u
#define MDEMOD_STRIP_BAD_HEADER      2u
#define MDEMOD_STRIP_TRUNCATED       4u
#define MDEMOD_STRIP_OUTSIDE         8u

typedef struct {
	uint32_t vcid;                /* 5                                                                                                */
	uint32_t period;              /* 43: packets per strip row, all apids                                                             */
	uint32_t apids[3];            /* 64 65 66: the active channels, each 64 .. 69, no two alike                                       */
	uint32_t reserved;            /* 0                                                                                                */
	uint64_t piece_frames;        /* mdemod_image_decode_host copies pieces of this many frames (+ the overlap): 0 = 8192, <= 2^20    */
} mdemod_image_opts;

typedef struct {
	uint32_t start;               /* stream position of the header                                                                    */
	uint32_t length;              /* total, 7 .. 65 542                                                                               */
	uint16_t apid;
	uint16_t seq;
	uint32_t flags;               /* sequence flags | secondary-header flag << 2                                                      */
} mdemod_packet;

typedef struct {
	uint8_t  mcus, q, mcun, flags;
	uint16_t day, us;
	uint32_t ms;
	uint32_t bits_used;
} mdemod_strip_info;

typedef struct {
	int32_t  channel;             /* slot 0 .. 2, or -1: not placed                                                                   */
	uint32_t row;                 /* strip row: line 8 row                                                                            */
	uint32_t cell;                /* mcun / 14: column 112 cell                                                                       */
	uint32_t reserved;
} mdemod_placement;

typedef struct {
	uint64_t packets;             /* descriptors                                                                                      */
	uint64_t per_apid[6];         /* image packets (no NOT_IMAGE / OUTSIDE) of apid 64 .. 69                                          */
	uint64_t placed, truncated, dropped;      /* candidates placed; of them truncated; candidates dropped                            */
	uint64_t seq_gaps;            /* among packets of apid 64 .. 70 in list order: places where seq is not the previous + 1           */
	uint64_t cells_filled;        /* over the three channels                                                                          */
	int64_t  first;               /* the anchor's `first`                                                                             */
	uint32_t rows;                /* strip rows: the height is 8 rows (0: no anchor)                                                  */
	uint32_t anchored;
} mdemod_place_summary;

/* What mdemod_image_decode_host returns: everything behind the pointers is malloc'ed, and mdemod_image_free gives it back. */
typedef struct {
	uint64_t n_packets;
	mdemod_packet *desc;          /* [n_packets], start relative to the whole batch                                                   */
	mdemod_strip_info *sinfo;     /* [n_packets]                                                                                      */
	uint8_t *strips;              /* [n_packets][8][112]                                                                              */
	mdemod_placement *place;      /* [n_packets]                                                                                      */
	mdemod_place_summary summary;
	uint8_t *image[3];            /* [8 rows][1568] per slot (NULL when rows = 0)                                                     */
	uint8_t *filled[3];           /* [rows][14]                                                                                       */
} mdemod_image_result;

/* vcid 5, period 43, apids 64 65 66, piece_frames 0. */
void mdemod_image_default_opts(mdemod_image_opts *opts);

/* vcdu_dev[n][892] and info_dev[n] (may be NULL: all frames good) into desc_dev[min(total, cap)] and *total_dev (a uint64: the
 * number of accepted packets, whatever cap is).  All device memory, at multiples of 4 bytes (total_dev: of 8).  Queued on hip_stream
 * of `device`; asynchronous; the scan's scratch memory is the call's own and freed in stream order.  n = 0: *total_dev := 0.  At
 * most 2^20 frames.  Nothing outside the inputs is read and nothing outside the outputs is written.  MDEMOD_ERR_PARAM (text in
 * mdemod_last_error) for a null or misaligned pointer, an option out of range, or ranges that intersect. */
int  mdemod_packets_find_device(const mdemod_image_opts *opts, const uint8_t *vcdu_dev, const mdemod_rs_info *info_dev, uint64_t n,
                                mdemod_packet *desc_dev, uint64_t cap, uint64_t *total_dev, int device, void *hip_stream);

/* desc_dev[n_desc] over vcdu_dev[n][892] into strips_dev[n_desc][8][112] and sinfo_dev[n_desc].  Asynchronous, as above.  A
 * descriptor that points outside the batch is reported (MDEMOD_STRIP_OUTSIDE), never followed.  n_desc = 0 is nothing to do. */
int  mdemod_image_decode_device(const mdemod_image_opts *opts, const uint8_t *vcdu_dev, uint64_t n, const mdemod_packet *desc_dev,
                                uint64_t n_desc, uint8_t *strips_dev, mdemod_strip_info *sinfo_dev, int device, void *hip_stream);

/* Host only: place[n_desc] and *summary (either may be NULL) from the descriptors and the reports, by the placement rule. */
int  mdemod_image_place(const mdemod_image_opts *opts, const mdemod_packet *desc, const mdemod_strip_info *sinfo, uint64_t n_desc,
                        mdemod_placement *place, mdemod_place_summary *summary);

/* VCDUs (and their reports, or NULL) in host memory to packets, strips and pictures.  Synchronous.  The frames are copied in pieces
 * of opts->piece_frames, each followed by MDEMOD_IMAGE_OVERLAP frames of the next, and a piece keeps the packets that start in
 * its own frames: the result is byte for byte that of one batch.  *out is overwritten; mdemod_image_free(out) afterwards. */
int  mdemod_image_decode_host(const mdemod_image_opts *opts, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n,
                              mdemod_image_result *out, int device);
void mdemod_image_free(mdemod_image_result *out);

#ifdef __cplusplus
}
#endif
#endif
