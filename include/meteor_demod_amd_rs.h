/*
 * meteor_demod_amd_rs.h — from CADUs to transfer frames (VCDUs, 892 bytes each): derandomising and Reed-Solomon correction.
 *
 * The frame layer (include/meteor_demod_amd_frames.h) ends in CADUs: the 4-byte marker and 1020 bytes that are XORed with the
 * CCSDS pseudo-noise sequence and carry four interleaved Reed-Solomon (255,223) codewords.  This layer takes the sequence off,
 * corrects every codeword (GPU, one block per CADU) and says for every frame how many bytes each codeword needed, or that it is
 * beyond the code.  The specification of the kernel is a host model (csrc/rs_host.cpp, exported as mdemod_rs_model_*,
 * csrc/rs_host.h): everything is integer arithmetic, and GPU bytes equal model bytes.
 *
 *   field       GF(256), polynomial x^8 + x^7 + x^2 + x + 1 (0x187), alpha = 0x02.
 *   code        RS(255,223), t = 16.  The generator's roots are alpha^(11 j), j = 112 .. 143; it is self-reciprocal; its coefficients
 *               from x^0 to x^32 are 01 5b 7f 56 10 1e 0d eb 61 a5 08 2a 36 56 ab 20 71 20 ab 56 36 2a 08 a5 61 eb 0d 1e 10 56 7f 5b 01
 *               (as powers of alpha the first half is 0 249 59 66 4 43 126 251 97 30 3 213 50 66 170 5 24).  A codeword is
 *               c[0 .. 254], c[0] the coefficient of x^254; c[0 .. 222] is data, c[223 .. 254] parity (systematic).  The data bytes
 *               0, 1, ..., 222 have the parity 2fbd4fb4748494b9acd554627212eeb3ebed41191de1d36320ea49290b25abcf.
 *   interleave  depth 4: byte i (0 .. 1019) after the marker is c[i / 4] of codeword i % 4.  The first 892 bytes are the VCDU in its
 *               natural order, the last 128 are parity.
 *   randomiser  an 8-bit register starts at 0xFF at every frame; per bit the output is bit 7, and after a shift left the new bit 0 is
 *               b7 ^ b4 ^ b2 ^ b0 (of the register before the shift); eight outputs form one byte, MSB first.  The sequence has a
 *               period of 255 bytes and begins ff 48 0e c0 9a 0d 70 bc.  Byte i of the 1020 is XORed with pn[i % 255]; the marker
 *               is not touched.
 *   decoding    a received word is corrected if and only if a codeword lies within Hamming distance 16 of it (that codeword is
 *               unique: the code's minimum distance is 33).  The output is that codeword and `corrected` the distance: the number of
 *               changed bytes, parity included.  Otherwise the word is left exactly as received (derandomised) and corrected = 255.
 *   options     derandomise (default 1; 0: the bytes are taken as they are).  dual_basis (default 0: the conventional representation,
 *               what the open LRPT decoders use for Meteor-M).  With dual_basis = 1 each derandomised byte b goes through Tinv[b]
 *               before decoding and each output byte v through T[v]: T[i] is the XOR of tal[7 - j] over the set bits j of i,
 *               tal = 8d ef ec 86 fa 99 af 7b; T is a permutation and begins 00 7b af d4 99 e2 36 4d fa 81 55 2e 63 18 cc b7.  Counts
 *               are unaffected.
 *   report      per frame: corrected[c] of codeword c = 0 .. 3, and flags: MDEMOD_RS_UNCORRECTABLE when any of them reads 255.  The
 *               other codewords of such a frame are still corrected.
 *   header      the first six bytes of a VCDU: version = b0 >> 6, spacecraft = ((b0 & 0x3f) << 2) | (b1 >> 6), vcid = b1 & 0x3f,
 *               counter = b2 b3 b4, big endian.
 */
#ifndef METEOR_DEMOD_AMD_RS_H
#define METEOR_DEMOD_AMD_RS_H

#include "meteor_demod_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_RS_CADU_BYTES        1024
#define MDEMOD_RS_VCDU_BYTES        892
#define MDEMOD_RS_T                 16      /* byte errors a codeword can lose */
#define MDEMOD_RS_FAILED            255     /* corrected[c] of a codeword that lies further than 16 from every codeword */
#define MDEMOD_RS_UNCORRECTABLE     1u      /* flags: at least one codeword of the frame reads 255 */
#define MDEMOD_RS_DEFAULT_PIECE     8192
#define MDEMOD_RS_MAX_PIECE         (1u << 20)

typedef struct {
	uint32_t derandomise;         /* 1 (default): the 1020 bytes are XORed with the pseudo-noise sequence first; 0: taken as they are  */
	uint32_t dual_basis;          /* 0 (default): conventional representation; 1: the CCSDS dual basis (Tinv before, T after)         */
	uint64_t piece_frames;        /* mdemod_rs_decode_host copies pieces of this many frames: 0 = 8192, at most 2^20                  */
} mdemod_rs_opts;

typedef struct {
	uint8_t  corrected[4];        /* per codeword: 0 .. 16 bytes changed, or 255                                                      */
	uint32_t flags;               /* MDEMOD_RS_UNCORRECTABLE                                                                          */
} mdemod_rs_info;

typedef struct {
	uint32_t version;
	uint32_t spacecraft;
	uint32_t vcid;
	uint32_t counter;
} mdemod_rs_header;

/* derandomise 1, dual_basis 0, piece_frames 0. */
void mdemod_rs_default_opts(mdemod_rs_opts *opts);

/* cadu_dev[n][1024] into vcdu_dev[n][892] and info_dev[n] (all device memory, all three at addresses that are multiples of 4).
 * Queued on hip_stream of `device`; asynchronous.  opts may be NULL (defaults).  n = 0 is nothing to do, not an error.  Nothing
 * outside cadu_dev[0 .. n) is read and nothing outside the two outputs is written.  MDEMOD_ERR_PARAM (text in mdemod_last_error)
 * for a null or misaligned pointer, an option out of range, or ranges that intersect. */
int  mdemod_rs_decode_device(const mdemod_rs_opts *opts, const uint8_t *cadu_dev, uint64_t n, uint8_t *vcdu_dev, mdemod_rs_info *info_dev,
                             int device, void *hip_stream);

/* The same for CADUs in host memory, copied in pieces of opts->piece_frames frames.  Synchronous.  The result is byte for byte that
 * of mdemod_rs_decode_device on the whole batch. */
int  mdemod_rs_decode_host(const mdemod_rs_opts *opts, const uint8_t *cadu, uint64_t n, uint8_t *vcdu, mdemod_rs_info *info, int device);

/* Host only: the header fields of one VCDU (its first five bytes are read). */
void mdemod_rs_vcdu_header(const uint8_t *vcdu, mdemod_rs_header *out);

#ifdef __cplusplus
}
#endif
#endif
