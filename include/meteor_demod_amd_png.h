/*
 * meteor_demod_amd_png.h — PNG (8 bit, no interlace) of a picture, lossless, with the `valid` mask of a map as transparency: every
 * picture, map and mosaic of the library as the file every other LRPT decoder writes.  The stream is fully determined by the picture,
 * the mask, `filter` and `segment`; the specification is a host model (csrc/png_host.cpp, exported as mdemod_png_model_*): GPU bytes
 * equal model bytes.
 *
 *   picture     uint8 [height][width][planes], planes 1 or 3.  width 1 .. 8192, height 1 .. 16 384.  valid: uint8 [height][width] or
 *               none; non-zero means valid.  Without a mask the colour type is 0 (grey) or 2 (RGB); with one it is 4 or 6 and the
 *               alpha byte behind a pixel's planes is 255 where valid != 0, else 0.  channels = planes (+ 1 with a mask).  Bit depth 8,
 *               no interlace, no palette, no ancillary chunk.
 *   filter      a row is its filter byte and width x channels bytes.  x: the byte, a: the byte `channels` before it in the row, b: the
 *               byte above it, c: the byte `channels` before b; what lies outside the picture is 0.  0 None x; 1 Sub x - a; 2 Up x - b;
 *               3 Average x - ((a + b) >> 1); 4 Paeth x - (p = a + b - c; the one of a, b, c nearest to p, ties in that order); all
 *               mod 256.  `filter` 0 .. 4: that filter for every row.  `filter` 5: per row the filter whose bytes v, read as signed
 *               (v < 128 ? v : 256 - v), have the smallest sum; ties go to the lower number.  The filtered stream is
 *               height x (1 + width x channels) bytes, N in all.
 *   segments    the filtered stream is cut every `segment` KiB (1 .. 32, 0 = 32) regardless of rows; the last may be short.  Segments
 *               are independent: no match reaches back across a segment start.
 *   parse       distance 1 only.  A run of L equal bytes inside a segment: its first byte is a literal; of the m = L - 1 others,
 *               matches of length 258 while 258 remain; a remainder of >= 3 is one match, a remainder of 1 or 2 is literals; m < 3:
 *               all literals.
 *   code        a segment is one dynamic-Huffman block (BFINAL 0) and an empty stored block (3 header bits, BFINAL 1 in the last
 *               segment, zero bits to the byte, 00 00 FF FF).  Literal/length counts: the tokens and one end-of-block.  Lengths:
 *                 order     the symbols with a count, ascending by (count, symbol): the leaves.
 *                 tree      Huffman by two queues, the leaves in that order and the made nodes in the order they were made; always the
 *                           two least weights, a leaf before a made node of equal weight.  A symbol's length is its leaf's depth.
 *                 limit     (15; 7 for the code-length code) n[l] = leaves of depth l, those deeper counted at the limit.  While
 *                           sum n[l] 2^(limit - l) exceeds 2^limit: n[limit] -= 1; the largest l < limit with n[l] > 0: n[l] -= 1,
 *                           n[l + 1] += 2.  Then the leaves in order (rarest first) take the lengths from the limit downwards, n[l]
 *                           leaves each.
 *               A complete prefix code; the codes are canonical (RFC 1951 3.2.2).  HLIT = the symbols up to the last with a length,
 *               257 at least.  HDIST = 1: distance code 0 with length 1, always (one code of one bit, which RFC 1951 allows; inflate
 *               accepts it with matches and without).  The HLIT + 1 lengths as one sequence, left to right: at a zero with r >= 3
 *               zeros from here (r counted to 138), 18 (r >= 11) or 17 with r; at a non-zero equal to the length before it with
 *               r >= 3 of them from here (counted to 6), 16 with r; else the length itself.  The code-length code by the same rule
 *               from those symbols' counts; HCLEN = up to the last with a length in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2
 *               14 1 15, 4 at least.
 *   fallback    if the dynamic block with its empty stored block is longer than len + 5 bytes, the segment is one stored block
 *               (BFINAL in the last; 1 + 2 + 2 bytes and the len bytes) and nothing else.  No fixed-Huffman blocks.
 *   file        signature; IHDR; an IDAT with the two zlib header bytes 78 01; one IDAT per segment; an IDAT with the Adler-32 of
 *               the filtered stream; IEND.  Every chunk has its own length and CRC-32.  47 bytes before the segments, 28 after.
 *   bound       47 + 28 + N + 17 per segment (a chunk's 12 bytes and the stored block's 5).
 */
#ifndef METEOR_DEMOD_AMD_PNG_H
#define METEOR_DEMOD_AMD_PNG_H

#include "meteor_demod_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_PNG_MAX_WIDTH    8192
#define MDEMOD_PNG_MAX_HEIGHT   16384
#define MDEMOD_PNG_MAX_SEGMENT  32         /* KiB; also what segment 0 stands for */
#define MDEMOD_PNG_FILTER_ADAPT 5          /* the least sum of absolute values, row by row */
#define MDEMOD_PNG_HEAD         47
#define MDEMOD_PNG_TAIL         28
#define MDEMOD_PNG_SEGMENT_OVERHEAD 17
#define MDEMOD_PNG_MAX_BYTES    (1ull << 30)   /* the most mdemod_png_deflate_device takes */

/* The largest file of such a picture (has_valid: with a mask); 0 for a size, planes or segment out of range. */
uint64_t mdemod_png_bound(uint32_t width, uint32_t height, uint32_t planes, uint32_t has_valid, uint32_t segment);
/* The largest output of mdemod_png_deflate_device for n_bytes bytes: n_bytes + 17 per segment; 0 out of range. */
uint64_t mdemod_png_deflate_bound(uint64_t n_bytes, uint32_t segment);

/* Bytes of workspace of mdemod_png_encode_device (the filtered stream; per segment its chunk, a length, an offset and two Adler sums)
 * and of mdemod_png_deflate_device (all but the first); 0 for arguments out of range. */
uint64_t mdemod_png_workspace(uint32_t width, uint32_t height, uint32_t planes, uint32_t has_valid, uint32_t segment);
uint64_t mdemod_png_deflate_workspace(uint64_t n_bytes, uint32_t segment);

/* picture_dev[height][width][planes] and valid_dev[height][width] (or NULL) into the file at out_dev[0 .. out_room), all in device
 * memory.  Queued on hip_stream of `device`; asynchronous; no host round trip.  result_dev[0] := the bytes of the file, always;
 * result_dev[1] := 1 when they fit out_room and are written, 0 when they do not: then no byte of out_dev is written.
 * work_dev[work_bytes] holds at least mdemod_png_workspace() bytes at a multiple of 16 bytes; result_dev stands at a multiple of 8
 * bytes.  Nothing outside the picture and the mask is read and nothing outside out_dev[0 .. out_room), the workspace and the result is
 * written.  MDEMOD_ERR_PARAM (text in mdemod_last_error) for a size, planes, filter or segment out of range, a missing or misaligned
 * pointer, a workspace that is too small, or buffers that intersect; nothing is written then. */
int  mdemod_png_encode_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment,
                              uint8_t *out_dev, uint64_t out_room, uint64_t *result_dev, void *work_dev, uint64_t work_bytes, int device, void *hip_stream);

/* The second stage alone: bytes_dev[n_bytes] (any bytes; 1 .. 2^30 of them, at a multiple of 16 bytes) into the segments' IDAT chunks
 * at out_dev[0 .. out_room): no head, no Adler chunk, no IEND; the last segment carries BFINAL.  result_dev as above.  Queued on
 * hip_stream of `device`; asynchronous. */
int  mdemod_png_deflate_device(const uint8_t *bytes_dev, uint64_t n_bytes, uint32_t segment, uint8_t *out_dev, uint64_t out_room, uint64_t *result_dev, void *work_dev,
                               uint64_t work_bytes, int device, void *hip_stream);

/* Waits for hip_stream and reads result_dev: *bytes := the bytes of the file (may be NULL).  MDEMOD_ERR_OVERFLOW, with the bytes
 * needed in the text, when they did not fit. */
int  mdemod_png_result(const uint64_t *result_dev, uint64_t *bytes, int device, void *hip_stream);

/* picture[height][width][planes] and valid[height][width] (or NULL) in host memory into a malloc'ed file: *file, *bytes;
 * mdemod_png_free gives it back.  Synchronous: uploads, encodes on `device`, downloads the file's bytes only. */
int  mdemod_png_encode_host(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment,
                            uint8_t **file, uint64_t *bytes, int device);
void mdemod_png_free(uint8_t *file);

#ifdef __cplusplus
}
#endif
#endif
