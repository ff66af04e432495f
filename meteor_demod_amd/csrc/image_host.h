/*
 * image_host.h — host side of the image layer (include/meteor_demod_amd_image.h): the tables (Huffman, zigzag, quantiser, the
 * transform's matrix; derived here, at compile time), the walk of one frame's packet headers and the decoding of one image packet,
 * written once for the host model (csrc/image_host.cpp, g++) and the kernels (csrc/image.hip): what differs between them - where a
 * lane keeps its block and its quantiser, how a strip is stored - comes in as a template parameter.  The check that is independent
 * of this file is tests/image_util.py.  Free of the GPU runtime.
 */
#ifndef MDEMOD_IMAGE_HOST_H
#define MDEMOD_IMAGE_HOST_H

#include "../../include/meteor_demod_amd_image.h"

#define IMG_ZONE      MDEMOD_IMAGE_ZONE_BYTES
#define IMG_VCDU      MDEMOD_RS_VCDU_BYTES
#define IMG_MAX_LEN   65542u
#define IMG_HEAD      20u                                  /* bytes of an image packet before its bit stream */
#define IMG_MAX_FRAMES (1u << 20)

#ifdef __cplusplus

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IMG_HD __host__ __device__ __forceinline__
#define IMG_UNROLL _Pragma("unroll")                       /* the small arrays below stay in registers only when their loops are unrolled */
#else
#define IMG_HD inline
#define IMG_UNROLL
#endif

/* cos table of the transform: c(j) = round(2^17 sqrt 2 cos(j pi / 16)) by the header's rule */
IMG_HD constexpr int32_t
img_c(int j)
{
	const int32_t N[9] = { 131072, 181802, 171254, 154124, 131072, 102983, 70936, 36163, 0 };
	j &= 31;
	if (j > 16) j = 32 - j;
	return j <= 8 ? N[j] : -N[16 - j];
}
IMG_HD constexpr int32_t img_m(int x, int u) { return u ? img_c((2 * x + 1) * u) : 131072; }

struct alignas(16) ImgTables {
	uint8_t  zigzag[64];
	uint8_t  std_q[64];
	uint8_t  dc_val[16];
	uint8_t  ac_val[176];
	int32_t  dc_max[17], dc_off[17];      /* a code of length L is in the table when code <= max[L]; its symbol is val[code + off[L]] */
	int32_t  ac_max[17], ac_off[17];
};
struct ImgCodes {                         /* the sender's side of the same tables */
	uint16_t dc_code[12], ac_code[256];
	uint8_t  dc_size[12], ac_size[256];
};

constexpr uint8_t IMG_DC_BITS[16] = { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 };
constexpr uint8_t IMG_AC_BITS[16] = { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d };
constexpr uint8_t IMG_AC_VAL[162] = {
	0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
	0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
	0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
	0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
	0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
	0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
	0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa };
constexpr uint8_t IMG_STD_Q[64] = {
	16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
	18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 };
constexpr uint8_t IMG_ZIGZAG[64] = {
	0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
	35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

constexpr ImgTables
img_make_tables()
{
	ImgTables t{};
	for (int i = 0; i < 64; i++) { t.zigzag[i] = IMG_ZIGZAG[i]; t.std_q[i] = IMG_STD_Q[i]; }
	for (int i = 0; i < 12; i++) t.dc_val[i] = static_cast<uint8_t>(i);
	for (int i = 0; i < 162; i++) t.ac_val[i] = IMG_AC_VAL[i];
	for (int tab = 0; tab < 2; tab++) {
		const uint8_t *bits = tab ? IMG_AC_BITS : IMG_DC_BITS;
		int32_t *mx = tab ? t.ac_max : t.dc_max, *off = tab ? t.ac_off : t.dc_off;
		int32_t code = 0, k = 0;
		mx[0] = -1; off[0] = 0;
		for (int L = 1; L <= 16; L++) {
			off[L] = k - code;
			code += bits[L - 1];
			k += bits[L - 1];
			mx[L] = bits[L - 1] ? code - 1 : -1;
			code <<= 1;
		}
	}
	return t;
}

constexpr ImgCodes
img_make_codes()
{
	ImgCodes c{};
	for (int tab = 0; tab < 2; tab++) {
		const uint8_t *bits = tab ? IMG_AC_BITS : IMG_DC_BITS;
		int32_t code = 0, k = 0;
		for (int L = 1; L <= 16; L++) {
			for (int i = 0; i < bits[L - 1]; i++, k++, code++) {
				if (tab) { c.ac_code[IMG_AC_VAL[k]] = static_cast<uint16_t>(code); c.ac_size[IMG_AC_VAL[k]] = static_cast<uint8_t>(L); }
				else { c.dc_code[k] = static_cast<uint16_t>(code); c.dc_size[k] = static_cast<uint8_t>(L); }
			}
			code <<= 1;
		}
	}
	return c;
}

constexpr bool
img_matrix_is_sound()
{
	for (int x = 0; x < 4; x++) {
		int64_t row = 0;
		for (int u = 0; u < 8; u++) {
			if (img_m(7 - x, u) != ((u & 1) ? -img_m(x, u) : img_m(x, u))) return false;
			row += img_m(x, u) < 0 ? -img_m(x, u) : img_m(x, u);
		}
		if (row * 2048 + 2048 >= (1ll << 31)) return false;                       /* pass 1 and, with |hi| <= 957, pass 2 stay in 32 bits */
	}
	return true;
}
static_assert(img_matrix_is_sound(), "the transform's rows mirror each other and no sum passes 2^31");

/* ---- headers ---- */
IMG_HD uint32_t img_fhp(const uint8_t *v) { return ((v[8] & 7u) << 8) | v[9]; }
IMG_HD uint32_t img_counter(const uint8_t *v) { return (static_cast<uint32_t>(v[2]) << 16) | (static_cast<uint32_t>(v[3]) << 8) | v[4]; }

IMG_HD bool
img_usable(const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t f, uint32_t vcid)
{
	const uint8_t *v = vcdu + f * IMG_VCDU;
	if ((v[0] >> 6) != 1u || (v[1] & 0x3Fu) != vcid) return false;
	if (info && (info[f].flags & MDEMOD_RS_UNCORRECTABLE)) return false;
	const uint32_t p = img_fhp(v);
	return p == MDEMOD_IMAGE_NO_HEADER || p < IMG_ZONE;
}

/* frames f and f + 1 (both inside the batch) are linked */
IMG_HD bool
img_linked(const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t f, uint32_t vcid)
{
	return img_usable(vcdu, info, f, vcid) && img_usable(vcdu, info, f + 1, vcid) &&
	       img_counter(vcdu + (f + 1) * IMG_VCDU) == ((img_counter(vcdu + f * IMG_VCDU) + 1u) & 0xFFFFFFu);
}

IMG_HD uint32_t img_stream_byte(const uint8_t *vcdu, uint64_t p) { return vcdu[(p / IMG_ZONE) * IMG_VCDU + 10u + p % IMG_ZONE]; }

/* The walk of frame f by the demultiplexing rule: the number of packets accepted; their descriptors go to out[0 ..] when out is
 * not NULL and `room` says how many it takes. */
IMG_HD uint32_t
img_walk(const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, uint64_t f, uint32_t vcid, mdemod_packet *out, uint64_t room)
{
	if (!img_usable(vcdu, info, f, vcid)) return 0;
	uint32_t pos = img_fhp(vcdu + f * IMG_VCDU), count = 0;
	if (pos == MDEMOD_IMAGE_NO_HEADER) return 0;
	uint64_t linked_to = f;                                                       /* frames f .. linked_to are a chain of links */
	while (pos < IMG_ZONE) {
		const uint64_t s = f * IMG_ZONE + pos;
		/* the chain as far as `need`, or not */
		uint64_t need = (s + 5) / IMG_ZONE;
		bool ok = true;
		for (int round = 0; round < 2 && ok; round++) {
			while (ok && linked_to < need) {
				if (linked_to + 1 < n && img_linked(vcdu, info, linked_to, vcid)) linked_to++;
				else ok = false;
			}
			if (!ok || round) break;
			const uint32_t len = 7u + ((img_stream_byte(vcdu, s + 4) << 8) | img_stream_byte(vcdu, s + 5));
			need = (s + len - 1) / IMG_ZONE;
		}
		if (!ok) break;
		const uint32_t h0 = img_stream_byte(vcdu, s), h1 = img_stream_byte(vcdu, s + 1), h2 = img_stream_byte(vcdu, s + 2), h3 = img_stream_byte(vcdu, s + 3);
		const uint32_t len = 7u + ((img_stream_byte(vcdu, s + 4) << 8) | img_stream_byte(vcdu, s + 5));
		const uint64_t end = s + len, g = end / IMG_ZONE;
		const uint32_t e = static_cast<uint32_t>(end % IMG_ZONE);
		for (uint64_t k = f + 1; k < g && ok; k++) ok = img_fhp(vcdu + k * IMG_VCDU) == MDEMOD_IMAGE_NO_HEADER;
		if (ok && e > 0 && g > f) ok = img_fhp(vcdu + g * IMG_VCDU) == e;
		if (ok && e == 0 && g < n && img_linked(vcdu, info, g - 1, vcid)) ok = img_fhp(vcdu + g * IMG_VCDU) == 0;
		if (!ok) break;
		if (out && count < room) {
			mdemod_packet d;
			d.start = static_cast<uint32_t>(s);
			d.length = len;
			d.apid = static_cast<uint16_t>(((h0 & 7u) << 8) | h1);
			d.seq = static_cast<uint16_t>(((h2 & 0x3Fu) << 8) | h3);
			d.flags = (h2 >> 6) | (((h0 >> 3) & 1u) << 2);
			out[count] = d;
		}
		count++;
		pos += len;
	}
	return count;
}

/* ---- one image packet ---- */

/* the bytes of a packet from a stream position on, across frame boundaries */
struct ImgSrc {
	const uint8_t *p;
	uint32_t zone_left, remain;
	IMG_HD void open(const uint8_t *vcdu, uint64_t pos, uint32_t bytes)
	{
		const uint64_t f = pos / IMG_ZONE;
		const uint32_t o = static_cast<uint32_t>(pos % IMG_ZONE);
		p = vcdu + f * IMG_VCDU + 10u + o;
		zone_left = IMG_ZONE - o;
		remain = bytes;
	}
	IMG_HD uint32_t next()                                                        /* remain > 0 */
	{
		if (!zone_left) { p += 10; zone_left = IMG_ZONE; }
		zone_left--; remain--;
		return *p++;
	}
};

struct ImgBits {
	ImgSrc src;
	uint32_t acc, cnt, used;
	IMG_HD bool ensure(uint32_t k)                                                /* k <= 16 */
	{
		while (cnt < k) {
			if (!src.remain) return false;
			acc = (acc << 8) | src.next();
			cnt += 8;
		}
		return true;
	}
	IMG_HD uint32_t take(uint32_t k) { cnt -= k; used += k; return (acc >> cnt) & ((1u << k) - 1u); }
	/* one code: the symbol, or -1 (the stream ended, or 16 bits match nothing) */
	IMG_HD int32_t symbol(const int32_t *mx, const int32_t *off, const uint8_t *val)
	{
		int32_t code = 0;
		for (int L = 1; L <= 16; L++) {
			if (!ensure(1)) return -1;
			code = (code << 1) | static_cast<int32_t>(take(1));
			if (code <= mx[L]) return val[code + off[L]];
		}
		return -1;
	}
	/* s extra bits, extended; ok := 0 when the stream ends */
	IMG_HD int32_t extra(uint32_t s, bool &ok)
	{
		if (!s) return 0;
		if (!ensure(s)) { ok = false; return 0; }
		const int32_t v = static_cast<int32_t>(take(s));
		return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
	}
};

IMG_HD uint32_t
img_quant(const ImgTables &T, uint32_t q, uint32_t i)
{
	const uint32_t sd = T.std_q[i];
	uint32_t v;
	if (q > 20 && q < 50) v = (5000u * sd + 50u * q) / (100u * q);
	else {
		const int32_t F = 200 - 2 * static_cast<int32_t>(q);
		v = F <= 0 ? 1u : (static_cast<uint32_t>(F) * sd + 50u) / 100u;
	}
	return v < 1u ? 1u : v;
}

/* S[x] = sum over u of M[x][u] a[u]: the even and the odd half once for x and 7 - x (the rows mirror each other) */
IMG_HD void
img_sums8(const int32_t *a, int32_t *S)
{
	IMG_UNROLL
	for (int x = 0; x < 4; x++) {
		const int32_t E = img_m(x, 0) * a[0] + img_m(x, 2) * a[2] + img_m(x, 4) * a[4] + img_m(x, 6) * a[6];
		const int32_t O = img_m(x, 1) * a[1] + img_m(x, 3) * a[3] + img_m(x, 5) * a[5] + img_m(x, 7) * a[7];
		S[x] = E + O;
		S[7 - x] = E - O;
	}
}

/* Blk: int32 get(i), void set(i, v) - the lane's 64 coefficients.  Qt: uint32 get(i), void set(i, v) - its quantiser.
 * Out: void put(block, row, lo, hi) - pixels 0 .. 3 and 4 .. 7 of one row of one block, little endian; every row of every block is
 * put exactly once.  Returns the report. */
template <class Blk, class Qt, class Out>
IMG_HD mdemod_strip_info
img_decode_packet(const ImgTables &T, const uint8_t *vcdu, uint64_t n, const mdemod_packet &d, Blk blk, Qt qt, Out out)
{
	mdemod_strip_info si;
	si.mcus = 0; si.q = 0; si.mcun = 0; si.flags = 0; si.day = 0; si.us = 0; si.ms = 0; si.bits_used = 0;
	uint32_t done = 0;
	if (d.length < 7u || d.length > IMG_MAX_LEN || static_cast<uint64_t>(d.start) + d.length > n * IMG_ZONE) si.flags = MDEMOD_STRIP_OUTSIDE;
	else if (d.apid < 64 || d.apid > 69 || !(d.flags & 4u) || d.length < IMG_HEAD + 1u) si.flags = MDEMOD_STRIP_NOT_IMAGE;
	else {
		ImgBits b;
		b.src.open(vcdu, static_cast<uint64_t>(d.start) + 6u, d.length - 6u);
		b.acc = 0; b.cnt = 0; b.used = 0;
		uint32_t h[14];
		IMG_UNROLL
		for (int i = 0; i < 14; i++) h[i] = b.src.next();
		si.day = static_cast<uint16_t>((h[0] << 8) | h[1]);
		si.ms = (h[2] << 24) | (h[3] << 16) | (h[4] << 8) | h[5];
		si.us = static_cast<uint16_t>((h[6] << 8) | h[7]);
		si.mcun = static_cast<uint8_t>(h[8]);
		si.q = static_cast<uint8_t>(h[13]);
		if (h[8] % 14u || h[8] > 182u || ((h[11] << 8) | h[12]) != 0xFFF0u) si.flags |= MDEMOD_STRIP_BAD_HEADER;
		for (uint32_t i = 0; i < 64; i++) qt.set(i, img_quant(T, h[13], i));
		int32_t dc = 0;
		for (; done < MDEMOD_IMAGE_MCUS; done++) {
			for (uint32_t i = 0; i < 64; i++) blk.set(i, 0);
			bool ok = true;
			int32_t sym = b.symbol(T.dc_max, T.dc_off, T.dc_val);
			if (sym < 0) break;
			dc += b.extra(static_cast<uint32_t>(sym), ok);
			if (!ok) break;
			{
				int32_t v = dc * static_cast<int32_t>(qt.get(0));
				blk.set(0, v < -2048 ? -2048 : v > 2047 ? 2047 : v);
			}
			uint32_t k = 1;
			while (k < 64) {
				sym = b.symbol(T.ac_max, T.ac_off, T.ac_val);
				if (sym < 0) { ok = false; break; }
				if (sym == 0) break;
				if (sym == 0xF0) { k += 16; if (k > 64) ok = false; continue; }
				k += static_cast<uint32_t>(sym) >> 4;
				if (k > 63) { ok = false; break; }
				const uint32_t z = T.zigzag[k];
				int32_t v = b.extra(static_cast<uint32_t>(sym) & 15u, ok);
				if (!ok) break;
				v *= static_cast<int32_t>(qt.get(z));
				blk.set(z, v < -2048 ? -2048 : v > 2047 ? 2047 : v);
				k++;
			}
			if (!ok) break;
			si.bits_used = b.used;
			/* pass 1: columns, in place */
			for (int u = 0; u < 8; u++) {
				int32_t a[8], S[8];
				IMG_UNROLL
				for (int v = 0; v < 8; v++) a[v] = blk.get(8 * v + u);
				img_sums8(a, S);
				IMG_UNROLL
				for (int y = 0; y < 8; y++) blk.set(8 * y + u, (S[y] + 2048) >> 12);
			}
			/* pass 2: rows */
			for (int y = 0; y < 8; y++) {
				int32_t hi[8], lo[8], A[8], B[8];
				IMG_UNROLL
				for (int u = 0; u < 8; u++) { const int32_t t = blk.get(8 * y + u); hi[u] = t >> 9; lo[u] = t & 511; }
				img_sums8(hi, A);
				img_sums8(lo, B);
				uint32_t w[2] = { 0, 0 };
				IMG_UNROLL
				for (int x = 0; x < 8; x++) {
					const int32_t R = A[x] + ((B[x] + 256) >> 9);
					int32_t p = 128 + ((R + 32768) >> 16);
					p = p < 0 ? 0 : p > 255 ? 255 : p;
					w[x >> 2] |= static_cast<uint32_t>(p) << (8 * (x & 3));
				}
				out.put(done, y, w[0], w[1]);
			}
		}
		si.mcus = static_cast<uint8_t>(done);
		if (done < MDEMOD_IMAGE_MCUS) si.flags |= MDEMOD_STRIP_TRUNCATED;
	}
	for (uint32_t k = done; k < MDEMOD_IMAGE_MCUS; k++)
		for (int y = 0; y < 8; y++) out.put(k, y, 0u, 0u);
	return si;
}

/* opts (NULL = defaults) checked: MDEMOD_OK or MDEMOD_ERR_PARAM with the text noted; piece_frames 0 becomes 8192 */
int  img_settings(const mdemod_image_opts *opts, mdemod_image_opts &out);

/* One piece of the host entry: k frames into descriptors (start relative to the piece), reports and strips. */
typedef int (*img_piece_fn)(void *ctx, const mdemod_image_opts &o, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t k,
                            std::vector<mdemod_packet> &desc, std::vector<mdemod_strip_info> &sinfo, std::vector<uint8_t> &strips);
/* The host entry around `piece` (the device's in csrc/image.hip, the model's here): the pieces, their overlap, the placement, the
 * pictures. */
int  img_decode_pieces(const mdemod_image_opts &o, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, mdemod_image_result *out,
                       img_piece_fn piece, void *ctx);

extern "C" {
#endif

/* ---- the host model: what the kernels of csrc/image.hip must compute, byte for byte (exported for the tests) ---- */

/* *total := the accepted packets of vcdu[n][892] (info may be NULL); desc[min(total, cap)] written */
int  mdemod_image_model_find(const mdemod_image_opts *opts, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, mdemod_packet *desc,
                             uint64_t cap, uint64_t *total);
/* desc[n_desc] into strips[n_desc][8][112] and sinfo[n_desc] */
int  mdemod_image_model_decode(const mdemod_image_opts *opts, const uint8_t *vcdu, uint64_t n, const mdemod_packet *desc, uint64_t n_desc,
                               uint8_t *strips, mdemod_strip_info *sinfo);
/* out[64] := the quantiser of q, by 8 row + column */
void mdemod_image_model_quant(uint32_t q, uint16_t *out);
/* out[64] := the pixels of in[64] (both by 8 row + column; in is saturated to -2048 .. 2047 first): the header's sums, term by term */
void mdemod_image_model_idct(const int32_t *in, uint8_t *out);
/* the tables as the decoder holds them: bits[2][16], dc_val[12], ac_val[162], zigzag[64], std[64], m[8][8] */
void mdemod_image_model_tables(uint8_t *bits, uint8_t *dc_val, uint8_t *ac_val, uint8_t *zigzag, uint8_t *std_q, int32_t *m);
/* The synthetic sender: one strip[8][112] into a whole packet (header included) at out[0 .. cap); returns its length, or a
 * negative status.  Sequence flags 3, secondary-header flag set, scan header 0, segment header 0xFFF0.  Its forward transform is
 * double precision and not part of the specification; its output is a valid stream. */
int64_t mdemod_image_model_encode_packet(const uint8_t *strip, uint32_t q, uint32_t mcun, uint32_t apid, uint32_t seq, uint32_t day, uint32_t ms,
                                         uint32_t us, uint8_t *out, uint64_t cap);
/* mdemod_image_decode_host with the model in the place of the kernels (no device) */
int  mdemod_image_model_host(const mdemod_image_opts *opts, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, mdemod_image_result *out);

#ifdef __cplusplus
}
#endif
#endif
