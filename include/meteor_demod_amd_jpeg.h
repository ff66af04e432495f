/*
 * meteor_demod_amd_jpeg.h — baseline sequential JPEG (SOF0, 8 bit, JFIF 1.01) of a picture: every picture, map and mosaic of the
 * library as a file that a browser and a GIS read.  The stream is fully determined by the picture, the quality and the restart
 * interval; the specification is a host model (csrc/jpeg_host.cpp, exported as mdemod_jpeg_model_*): GPU bytes equal model bytes.
 *
 *   picture     uint8 [height][width][planes], planes 1 (one component) or 3 (R, G, B; coded as Y, Cb, Cr at 4:4:4, one block of
 *               each per MCU in that order).  width 1 .. 8192, height 1 .. 16 384.  An MCU covers 8 x 8 pixels; the last column and
 *               the last line are repeated up to the next multiple of 8.  MCUs count in raster order.
 *   colour      integers, 16-bit fixed point (libjpeg's FIX() constants and its chroma offset), >> is a floor:
 *                 Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *                 Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *                 Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16
 *               each within 0 .. 255.  A grey picture's byte is its Y.  The level shift takes 128 from every sample: f = s - 128.
 *   transform   32-bit integers.  c(j) = round(2^17 sqrt 2 cos(j pi / 16)) = 131072, 181802, 171254, 154124, 131072, 102983, 70936,
 *               36163, 0 for j = 0 .. 8 (the table of the image layer), M[x][0] = 131072, M[x][u] = c((2 x + 1) u) with the cosine's
 *               symmetries.  Lines first: t[y][u] = (sum over x of f[y][x] M[x][u] + 512) >> 10.  Then columns, with t split so
 *               that no sum passes 2^31: hi = t >> 9, lo = t & 511,
 *                 R[v][u] = sum over y of hi[y][u] M[y][v] + ((sum over y of lo[y][u] M[y][v] + 256) >> 9).
 *               R is the coefficient of the orthonormal 8 x 8 DCT times 2^18 (|t| <= 2^17, |R| < 2^28.1: a column of M sums to
 *               2^20 at most in absolute value, and |f| <= 128).
 *   quantiser   base tables of Annex K.1 (Y, grey) and K.2 (Cb, Cr), natural order.  quality q = 1 .. 100, S = 5000 / q (integer
 *               division) below 50, else 200 - 2 q; Q = clamp((base S + 50) / 100, 1, 255).  The level is
 *                 sign(R) ((|R| + (Q << 17)) / (Q << 18)):  R / (2^18 Q) rounded to the nearest, halves away from zero,
 *               then clamped: the DC level to -1024 .. 1023 (a DC difference is of category 11 at most), an AC level to
 *               -1023 .. 1023 (category 10 at most).  The entropy coder clamps what it is given in the same way.
 *   coef        int16 [blocks][64], the 64 levels of a block in zig-zag order, the blocks of an MCU adjacent (Y, Cb, Cr), the MCUs in
 *               raster order.
 *   entropy     the four tables of Annex K.3 - K.6, always.  restart interval Ri = 1 .. 64 MCUs (0 = 32): segment s holds the MCUs
 *               s Ri .. min((s + 1) Ri, n) - 1 (a segment may run across the end of an MCU row; the last may be short); the DC
 *               prediction of every component begins at 0 in every segment; the segment's bits, most significant first, are
 *               padded with 1-bits to a byte, and every FF byte is followed by a 00; RSTm (FF D0 + m), m = s mod 8, stands
 *               between segment s and segment s + 1.
 *               A block is at most 22 bits of DC (a code of 11 bits in K.4, 11 more bits; 9 + 11 in K.3) and 63 x 26 bits of AC (a
 *               code of 16 bits, 10 more bits; a ZRL spends 11 bits on 16 coefficients, which is less): 1660 bits, 208 bytes.  A
 *               segment is at most 208 Ri planes bytes before the 00s and twice that after: MDEMOD_JPEG_BLOCK_BYTES.
 *   file        SOI; APP0 "JFIF" 1.01, density 1 : 1 without a unit, no thumbnail; one DQT with table 0 (and table 1 for colour),
 *               8 bit, zig-zag order; SOF0 (components 1, 2, 3, sampling 1 x 1, tables 0, 1, 1); one DHT with DC 0, AC 0 (and
 *               DC 1, AC 1); DRI; SOS (Ss 0, Se 63, Ah Al 0); the segments; EOI.  330 bytes before the segments for a grey
 *               picture, 613 for a colour one.
 */
#ifndef METEOR_DEMOD_AMD_JPEG_H
#define METEOR_DEMOD_AMD_JPEG_H

#include "meteor_demod_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_JPEG_MAX_WIDTH    8192
#define MDEMOD_JPEG_MAX_HEIGHT   16384
#define MDEMOD_JPEG_MAX_RESTART  64
#define MDEMOD_JPEG_RESTART      32         /* what restart_interval 0 stands for */
#define MDEMOD_JPEG_BLOCK_BYTES  208        /* the bits of one block fit these bytes (before the 00 bytes) */
#define MDEMOD_JPEG_HEAD_GREY    330
#define MDEMOD_JPEG_HEAD_COLOUR  613

/* The largest file of such a picture: head + 2 x 208 bytes per block + 2 per segment (markers, EOI).  0 for a size, planes or
 * interval out of range. */
uint64_t mdemod_jpeg_bound(uint32_t width, uint32_t height, uint32_t planes, uint32_t restart_interval);
/* The largest output of mdemod_jpeg_entropy_device for n_mcus MCUs; 0 for planes or an interval out of range. */
uint64_t mdemod_jpeg_entropy_bound(uint64_t n_mcus, uint32_t planes, uint32_t restart_interval);

/* Bytes of workspace of mdemod_jpeg_encode_device (the coefficients, a length and an offset per segment) and of
 * mdemod_jpeg_entropy_device (the latter two); 0 for arguments out of range. */
uint64_t mdemod_jpeg_workspace(uint32_t width, uint32_t height, uint32_t planes, uint32_t restart_interval);
uint64_t mdemod_jpeg_entropy_workspace(uint64_t n_mcus, uint32_t restart_interval);

/* picture_dev[height][width][planes] into the file at out_dev[0 .. out_room), all in device memory.  Queued on hip_stream of
 * `device`; asynchronous.  result_dev[0] := the bytes of the file, always; result_dev[1] := 1 when they fit out_room and are
 * written, 0 when they do not: then no byte of out_dev is written.  work_dev[work_bytes] holds at least mdemod_jpeg_workspace()
 * bytes at a multiple of 16 bytes; result_dev stands at a multiple of 8 bytes.  Nothing outside the picture is read and nothing
 * outside out_dev[0 .. out_room), the workspace and the result is written.  MDEMOD_ERR_PARAM (text in mdemod_last_error) for a size,
 * planes, quality or interval out of range, a missing or misaligned pointer, a workspace that is too small, or outputs that
 * intersect each other or the picture; nothing is written then. */
int  mdemod_jpeg_encode_device(const uint8_t *picture_dev, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval,
                               uint8_t *out_dev, uint64_t out_room, uint64_t *result_dev, void *work_dev, uint64_t work_bytes, int device, void *hip_stream);

/* The second stage alone: coef_dev[n_mcus planes][64] (any int16; clamped as the header says) into the segments and the RSTm
 * between them at out_dev[0 .. out_room): no head, no EOI.  result_dev as above.  coef_dev and work_dev at multiples of 16 bytes,
 * n_mcus 1 .. 2^21.  Queued on hip_stream of `device`; asynchronous. */
int  mdemod_jpeg_entropy_device(const int16_t *coef_dev, uint64_t n_mcus, uint32_t planes, uint32_t restart_interval, uint8_t *out_dev, uint64_t out_room,
                                uint64_t *result_dev, void *work_dev, uint64_t work_bytes, int device, void *hip_stream);

/* Waits for hip_stream and reads result_dev: *bytes := the bytes of the file (may be NULL).  MDEMOD_ERR_OVERFLOW, with the bytes
 * needed in the text, when they did not fit. */
int  mdemod_jpeg_result(const uint64_t *result_dev, uint64_t *bytes, int device, void *hip_stream);

/* picture[height][width][planes] in host memory into a malloc'ed file: *file, *bytes; mdemod_jpeg_free gives it back.
 * Synchronous: uploads, encodes on `device`, downloads the file's bytes only. */
int  mdemod_jpeg_encode_host(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval,
                             uint8_t **file, uint64_t *bytes, int device);
void mdemod_jpeg_free(uint8_t *file);

#ifdef __cplusplus
}
#endif
#endif
