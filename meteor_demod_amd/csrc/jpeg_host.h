/*
 * jpeg_host.h — what the host model (csrc/jpeg_host.cpp, g++) and the kernels (csrc/jpeg.hip) of the JPEG encoder
 * (include/meteor_demod_amd_jpeg.h) share, written once: the tables (the luminance ones, the zig-zag order and the cosine table are the
 * image layer's, csrc/image_host.h; the chrominance ones of Annex K.2, K.4 and K.6 are here), the colour transform, the two passes
 * of the forward transform, the quantiser, and the coding of one block into a sink of (bits, count) pairs: the model's sink writes
 * bits, the kernels' sinks count them or put them into LDS.  The check that is independent of this file is tests/jpeg_ref.py.
 * Free of the GPU runtime.
 *
 * Every shift and rounding, in the order of the data:
 *   colour      (sum + 32768) >> 16 for Y, (sum + 8388608 + 32767) >> 16 for Cb and Cr; the sums are positive
 *   level       f = sample - 128
 *   lines       t = (sum + 512) >> 10, an arithmetic shift (a floor)
 *   columns     hi = t >> 9 (a floor), lo = t & 511, R = A + ((B + 256) >> 9)
 *   quantiser   (|R| + (Q << 17)) / (Q << 18), unsigned; the sign put back; the clamp
 */
#ifndef MDEMOD_JPEG_HOST_H
#define MDEMOD_JPEG_HOST_H

#include "../../include/meteor_demod_amd_jpeg.h"
#include "image_host.h"

#define JPG_HD IMG_HD
#define JPEG_HEAD_ROOM 640u                     /* the head of a file fits: 330 or 613 bytes */
#define JPEG_MAX_MCUS  (1ull << 21)             /* 8192 x 16 384 pixels */

constexpr uint8_t JPEG_CHROMA_Q[64] = {
	17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
	99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 };
constexpr uint8_t JPEG_DC_BITS_C[16] = { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 };
constexpr uint8_t JPEG_AC_BITS_C[16] = { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 };
constexpr uint8_t JPEG_AC_VAL_C[162] = {
	0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
	0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
	0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
	0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
	0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
	0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
	0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa };

/* the sender's side of the four tables: code | length << 16, by symbol; 0 where the table has no such symbol.  [0] K.3 / K.5
 * (luminance), [1] K.4 / K.6 (chrominance) */
struct JpegCodes {
	uint32_t dc[2][16];
	uint32_t ac[2][256];
};

constexpr JpegCodes
jpeg_make_codes()
{
	JpegCodes c{};
	for (int tab = 0; tab < 4; tab++) {
		const uint8_t *bits = tab == 0 ? IMG_DC_BITS : tab == 1 ? IMG_AC_BITS : tab == 2 ? JPEG_DC_BITS_C : JPEG_AC_BITS_C;
		const uint8_t *val = tab == 1 ? IMG_AC_VAL : JPEG_AC_VAL_C;
		uint32_t code = 0, k = 0;
		for (uint32_t L = 1; L <= 16; L++) {
			for (uint32_t i = 0; i < bits[L - 1]; i++, k++, code++) {
				if (tab & 1) c.ac[tab >> 1][val[k]] = code | (L << 16);
				else c.dc[tab >> 1][k] = code | (L << 16);
			}
			code <<= 1;
		}
	}
	return c;
}

/* where the coefficient at 8 v + u stands in zig-zag order */
struct JpegUnzig { uint8_t at[64]; };
constexpr JpegUnzig
jpeg_make_unzig()
{
	JpegUnzig z{};
	for (int k = 0; k < 64; k++) z.at[IMG_ZIGZAG[k]] = static_cast<uint8_t>(k);
	return z;
}

/* Q of `quality` for the base table's entry */
JPG_HD constexpr uint32_t
jpeg_quant(uint32_t quality, uint32_t base)
{
	const uint32_t S = quality < 50u ? 5000u / quality : 200u - 2u * quality;
	const uint32_t v = (base * S + 50u) / 100u;
	return v < 1u ? 1u : v > 255u ? 255u : v;
}

/* q[2][64], natural order: [0] luminance, [1] chrominance */
inline void
jpeg_quant_tables(uint32_t quality, uint8_t *q)
{
	for (int i = 0; i < 64; i++) {
		q[i] = static_cast<uint8_t>(jpeg_quant(quality, IMG_STD_Q[i]));
		q[64 + i] = static_cast<uint8_t>(jpeg_quant(quality, JPEG_CHROMA_Q[i]));
	}
}

/* component c (0 Y, 1 Cb, 2 Cr) of a pixel */
JPG_HD int32_t
jpeg_ycc(int c, int32_t r, int32_t g, int32_t b)
{
	if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
	if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
	return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

constexpr bool
jpeg_sums_fit()
{
	for (int u = 0; u < 8; u++) {
		int64_t column = 0;
		for (int x = 0; x < 4; x++) column += img_m(x, u) < 0 ? -img_m(x, u) : img_m(x, u);
		if (column * 1022 >= (1ll << 31)) return false;                          /* |a[x] +- a[7 - x]| <= 1022 */
	}
	return true;
}
static_assert(jpeg_sums_fit(), "no sum of jpeg_sums8 passes 2^31 while |a| <= 511");

/* S[u] = sum over x of M[x][u] a[x]: the rows of M mirror each other with the sign (-1)^u, so the even u take a[x] + a[7 - x] and
 * the odd ones a[x] - a[7 - x].  |a| <= 511 (samples: 128, hi: 256, lo: 511): no sum passes 2^31. */
JPG_HD void
jpeg_sums8(const int32_t *a, int32_t *S)
{
	int32_t s[4], d[4];
	IMG_UNROLL
	for (int x = 0; x < 4; x++) { s[x] = a[x] + a[7 - x]; d[x] = a[x] - a[7 - x]; }
	IMG_UNROLL
	for (int u = 0; u < 8; u++) {
		const int32_t *h = (u & 1) ? d : s;
		S[u] = img_m(0, u) * h[0] + img_m(1, u) * h[1] + img_m(2, u) * h[2] + img_m(3, u) * h[3];
	}
}

/* one line of a block: 8 level-shifted samples into t[0 .. 7] */
JPG_HD void
jpeg_line(const int32_t *f, int32_t *t)
{
	int32_t S[8];
	jpeg_sums8(f, S);
	IMG_UNROLL
	for (int u = 0; u < 8; u++) t[u] = (S[u] + 512) >> 10;
}

/* one column of a block: t[0 .. 7] of the lines y into R[0 .. 7] of the frequencies v */
JPG_HD void
jpeg_column(const int32_t *t, int32_t *R)
{
	int32_t hi[8], lo[8], A[8], B[8];
	IMG_UNROLL
	for (int y = 0; y < 8; y++) { hi[y] = t[y] >> 9; lo[y] = t[y] & 511; }
	jpeg_sums8(hi, A);
	jpeg_sums8(lo, B);
	IMG_UNROLL
	for (int v = 0; v < 8; v++) R[v] = A[v] + ((B[v] + 256) >> 9);
}

/* the level of R under Q, clamped; dc: the block's first coefficient */
JPG_HD int32_t
jpeg_level(int32_t R, uint32_t Q, bool dc)
{
	const uint32_t a = R < 0 ? 0u - static_cast<uint32_t>(R) : static_cast<uint32_t>(R);
	int32_t v = static_cast<int32_t>((a + (Q << 17)) / (Q << 18));
	if (R < 0) v = -v;
	const int32_t low = dc ? -1024 : -1023;
	return v < low ? low : v > 1023 ? 1023 : v;
}

/* One block into `sink`: sink.put(bits, count) takes `count` <= 27 bits, the most significant first.  Src: void load8(g, int16 v[8]),
 * the coefficients 8 g .. 8 g + 7 in zig-zag order.  dc[16] and ac[256] are the component's codes.  Returns the block's DC level
 * after the clamp, the next block's prediction. */
template <class Src, class Sink>
JPG_HD int32_t
jpeg_code_block(const uint32_t *dc, const uint32_t *ac, const Src &src, int32_t pred, Sink &sink)
{
	int32_t first = 0;
	uint32_t run = 0;
	for (int g = 0; g < 8; g++) {
		int16_t w[8];
		src.load8(g, w);
		IMG_UNROLL
		for (int j = 0; j < 8; j++) {
			int32_t v = w[j];
			if (g == 0 && j == 0) {
				v = v < -1024 ? -1024 : v > 1023 ? 1023 : v;
				first = v;
				const int32_t diff = v - pred;
				const uint32_t a = static_cast<uint32_t>(diff < 0 ? -diff : diff);
				const uint32_t s = a ? 32u - static_cast<uint32_t>(__builtin_clz(a)) : 0u;
				const uint32_t e = static_cast<uint32_t>(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u);
				const uint32_t code = dc[s];
				sink.put(((code & 0xFFFFu) << s) | e, (code >> 16) + s);
				continue;
			}
			v = v < -1023 ? -1023 : v > 1023 ? 1023 : v;
			if (!v) { run++; continue; }
			while (run >= 16) { sink.put(ac[0xF0] & 0xFFFFu, ac[0xF0] >> 16); run -= 16; }
			const uint32_t a = static_cast<uint32_t>(v < 0 ? -v : v);
			const uint32_t s = 32u - static_cast<uint32_t>(__builtin_clz(a));
			const uint32_t e = static_cast<uint32_t>(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
			const uint32_t code = ac[(run << 4) | s];
			sink.put(((code & 0xFFFFu) << s) | e, (code >> 16) + s);
			run = 0;
		}
	}
	if (run) sink.put(ac[0] & 0xFFFFu, ac[0] >> 16);
	return first;
}

/* the arguments of the two device entries and of the model's: MDEMOD_OK, or MDEMOD_ERR_PARAM with the text noted */
int  jpeg_check_picture(const char *who, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval);
int  jpeg_check_entropy(const char *who, uint64_t n_mcus, uint32_t planes, uint32_t restart_interval);
inline uint32_t jpeg_interval(uint32_t restart_interval) { return restart_interval ? restart_interval : MDEMOD_JPEG_RESTART; }
inline uint64_t jpeg_mcus(uint32_t width, uint32_t height) { return static_cast<uint64_t>((width + 7u) / 8u) * ((height + 7u) / 8u); }
/* the file's bytes before the first segment into head[JPEG_HEAD_ROOM]; returns their number */
uint32_t jpeg_head(uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval, uint8_t *head);

extern "C" {

/* ---- the host model: what the kernels of csrc/jpeg.hip must compute, byte for byte (exported for the tests) ---- */

/* q[2][64] := the quantisers of `quality` (luminance, chrominance; natural order); bits[4][16] and vals[4][162] := the tables K.3,
 * K.5, K.4, K.6 as a DHT holds them (vals of a DC table: 12 used); zigzag[64]; m[8][8] := M */
int  mdemod_jpeg_model_tables(uint32_t quality, uint8_t *q, uint8_t *bits, uint8_t *vals, uint8_t *zigzag, int32_t *m);
/* R[64] := the transform of samples[64] (0 .. 255, both by 8 row + column): 2^18 times the coefficient */
void mdemod_jpeg_model_fdct(const uint8_t *samples, int32_t *R);
/* coef[mcus planes][64] := the levels of the picture */
int  mdemod_jpeg_model_coefficients(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, int16_t *coef);
/* coef[n_mcus planes][64] into the segments and the markers between them: *bytes := their number, always; written when they fit
 * out_room, else MDEMOD_ERR_OVERFLOW and nothing written */
int  mdemod_jpeg_model_entropy(const int16_t *coef, uint64_t n_mcus, uint32_t planes, uint32_t restart_interval, uint8_t *out, uint64_t out_room,
                               uint64_t *bytes);
/* the whole file, as mdemod_jpeg_model_entropy gives its bytes */
int  mdemod_jpeg_model_encode(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval,
                              uint8_t *out, uint64_t out_room, uint64_t *bytes);

}

#endif
