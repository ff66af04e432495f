/*
 * png_host.h — what the host model (csrc/png_host.cpp, g++) and the kernels (csrc/png.hip) of the PNG encoder
 * (include/meteor_demod_amd_png.h) share, written once: the five filters, what stands at a place of a run, the length symbols, the
 * Huffman lengths with their limit, the run-length coding of the lengths, the header of a dynamic block into a sink of (bits, count)
 * pairs, the CRC-32 table and the multiplication that joins the CRCs of slices.  The check that is independent of this file is
 * tests/png_ref.py (zlib's inflate and crc32).  Free of the GPU runtime.
 */
#ifndef MDEMOD_PNG_HOST_H
#define MDEMOD_PNG_HOST_H

#include <cstdint>

#include "../../include/meteor_demod_amd_png.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNG_HD __host__ __device__ __forceinline__
#else
#define PNG_HD inline
#endif

#define PNG_LL        286                       /* literal/length symbols */
#define PNG_LL_ROOM   288                       /* (the distance length stands behind the last literal/length one) */
#define PNG_CL        19
#define PNG_EOB       256
#define PNG_ADLER     65521u
#define PNG_POLY      0xEDB88320u

/* ---- filters ---- */
PNG_HD uint32_t
png_paeth(uint32_t a, uint32_t b, uint32_t c)
{
	const int32_t p = static_cast<int32_t>(a + b) - static_cast<int32_t>(c);
	const int32_t pa = p > static_cast<int32_t>(a) ? p - static_cast<int32_t>(a) : static_cast<int32_t>(a) - p;
	const int32_t pb = p > static_cast<int32_t>(b) ? p - static_cast<int32_t>(b) : static_cast<int32_t>(b) - p;
	const int32_t pc = p > static_cast<int32_t>(c) ? p - static_cast<int32_t>(c) : static_cast<int32_t>(c) - p;
	return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

/* the byte x under filter f with its neighbours a (left), b (above), c (above left) */
PNG_HD uint32_t
png_filter_byte(uint32_t f, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
	const uint32_t pred = f == 0 ? 0u : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
	return (x - pred) & 255u;
}

/* what a filtered byte adds to its row's sum */
PNG_HD uint32_t png_cost(uint32_t v) { return v < 128u ? v : 256u - v; }

/* the filter of a row from the five sums */
PNG_HD uint32_t
png_choose(const uint32_t *sum)
{
	uint32_t best = 0;
	for (uint32_t f = 1; f < 5; f++)
		if (sum[f] < sum[best]) best = f;
	return best;
}

/* ---- parse ---- */
/* what stands at place k of a run of L equal bytes: 0 nothing (inside a match), 1 a literal, 3 .. 258 a match of that length */
PNG_HD uint32_t
png_token(uint32_t k, uint32_t L)
{
	if (k == 0 || L < 4) return 1;
	const uint32_t m = L - 1, j = k - 1, r = j % 258u, rem = m % 258u;
	if (j < m - rem) return r ? 0u : 258u;
	if (rem < 3) return 1;
	return r ? 0u : rem;
}

/* a match length 3 .. 258: its symbol less 257, and its extra bits (count and value) */
PNG_HD uint32_t
png_length_symbol(uint32_t length, uint32_t *extra_bits, uint32_t *extra)
{
	const uint32_t l = length - 3;
	if (length == 258) { *extra_bits = 0; *extra = 0; return 28; }
	if (l < 8) { *extra_bits = 0; *extra = 0; return l; }
	const uint32_t n = 31u - static_cast<uint32_t>(__builtin_clz(l)), e = n - 2;
	*extra_bits = e;
	*extra = l & ((1u << e) - 1u);
	return 4 * e + 4 + ((l >> e) & 3u);
}

/* ---- code lengths ---- */
/* is symbol a before symbol b among the leaves?  (both have a count) */
PNG_HD bool png_before(const uint32_t *count, uint32_t a, uint32_t b) { return count[a] < count[b] || (count[a] == count[b] && a < b); }

/* len[order[i]] := the length of leaf i, for the n leaves order[0 .. n) (ascending by png_before), by the header's rule.  len is
 * zero beforehand.  Scratch: w[2 n], up[2 n], num[16]. */
PNG_HD void
png_code_lengths(const uint32_t *count, const uint16_t *order, uint32_t n, uint32_t limit, uint8_t *len, uint32_t *w, uint16_t *up, uint32_t *num)
{
	if (n == 0) return;
	if (n == 1) { len[order[0]] = 1; return; }
	for (uint32_t i = 0; i < n; i++) w[i] = count[order[i]];
	uint32_t leaf = 0, made = n;
	for (uint32_t next = n; next < 2 * n - 1; next++) {
		uint32_t sum = 0;
		for (int t = 0; t < 2; t++) {
			const uint32_t pick = (leaf < n && (made >= next || w[leaf] <= w[made])) ? leaf++ : made++;
			up[pick] = static_cast<uint16_t>(next);
			sum += w[pick];
		}
		w[next] = sum;
	}
	up[2 * n - 2] = 0;                                                             /* from here on up[] is the depth */
	for (uint32_t i = 2 * n - 2; i-- > 0;) up[i] = static_cast<uint16_t>(up[up[i]] + 1);
	for (uint32_t l = 0; l <= limit; l++) num[l] = 0;
	for (uint32_t i = 0; i < n; i++) num[up[i] < limit ? up[i] : limit]++;
	uint32_t total = 0;
	for (uint32_t l = 1; l <= limit; l++) total += num[l] << (limit - l);
	while (total > (1u << limit)) {
		num[limit]--;
		for (uint32_t l = limit - 1; l > 0; l--)
			if (num[l]) { num[l]--; num[l + 1] += 2; break; }
		total--;
	}
	uint32_t i = 0;
	for (uint32_t l = limit; l > 0; l--)
		for (uint32_t c = num[l]; c; c--) len[order[i++]] = static_cast<uint8_t>(l);
}

/* the canonical code of symbol s (RFC 1951 3.2.2) with its bits reversed: as the stream holds it, first bit lowest */
PNG_HD uint32_t
png_code_of(const uint8_t *len, uint32_t n, uint32_t s)
{
	const uint32_t l = len[s];
	if (!l) return 0;
	uint32_t code = 0;                                                             /* (the first code of length l) + the symbols of length l below s */
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t li = len[i];
		if (li && li < l) code += 1u << (l - li);
		else if (li == l && i < s) code++;
	}
	uint32_t rev = 0;
	for (uint32_t b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
	return rev;
}

/* seq[0 .. n) into symbols of the code-length alphabet: tok[] := symbol | extra << 8; their counts are added to clcount[19].
 * Returns the number of symbols (n at most). */
PNG_HD uint32_t
png_rle(const uint8_t *seq, uint32_t n, uint16_t *tok, uint32_t *clcount)
{
	uint32_t i = 0, t = 0;
	while (i < n) {
		const uint32_t v = seq[i], cap = v ? 6u : 138u;
		uint32_t r = 1, sym = v, extra = 0, step = 1;
		while (r < cap && i + r < n && seq[i + r] == v) r++;
		if (v == 0 && r >= 3) { sym = r >= 11 ? 18 : 17; extra = r - (r >= 11 ? 11 : 3); step = r; }
		else if (v != 0 && i > 0 && seq[i - 1] == v && r >= 3) { sym = 16; extra = r - 3; step = r; }
		tok[t++] = static_cast<uint16_t>(sym | (extra << 8));
		clcount[sym]++;
		i += step;
	}
	return t;
}

PNG_HD uint32_t png_cl_extra_bits(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }
/* the order in which the code-length lengths are sent: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 */
PNG_HD uint32_t png_cl_order(uint32_t i)
{
	return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - (i - 3) / 2 : 8 + (i - 4) / 2;
}

/* HCLEN: the code-length lengths sent */
PNG_HD uint32_t
png_hclen(const uint8_t *cllen)
{
	uint32_t h = PNG_CL;
	while (h > 4 && !cllen[png_cl_order(h - 1)]) h--;
	return h;
}

/* the bits of a dynamic block before its first symbol */
PNG_HD uint32_t
png_header_bits(const uint16_t *tok, uint32_t n_tok, const uint8_t *cllen)
{
	uint32_t bits = 3 + 5 + 5 + 4 + 3 * png_hclen(cllen);
	for (uint32_t t = 0; t < n_tok; t++) bits += cllen[tok[t] & 255u] + png_cl_extra_bits(tok[t] & 255u);
	return bits;
}

/* those bits into sink.put(bits, count): the first bit lowest */
template <class Sink>
PNG_HD void
png_put_header(Sink &sink, uint32_t hlit, const uint16_t *tok, uint32_t n_tok, const uint8_t *cllen, const uint16_t *clcode)
{
	const uint32_t hclen = png_hclen(cllen);
	sink.put(0u | (2u << 1), 3);                                                   /* BFINAL 0, BTYPE 10 */
	sink.put(hlit - 257, 5);
	sink.put(0, 5);                                                                /* HDIST: one code */
	sink.put(hclen - 4, 4);
	for (uint32_t i = 0; i < hclen; i++) sink.put(cllen[png_cl_order(i)], 3);
	for (uint32_t t = 0; t < n_tok; t++) {
		const uint32_t sym = tok[t] & 255u, extra = tok[t] >> 8, l = cllen[sym];
		sink.put(clcode[sym] | (extra << l), l + png_cl_extra_bits(sym));
	}
}

/* one token into the sink: a literal `byte`, or a match of `token` bytes at distance 1 */
template <class Sink>
PNG_HD void
png_put_token(Sink &sink, uint32_t byte, uint32_t token, const uint8_t *len, const uint16_t *code)
{
	if (token == 1) { sink.put(code[byte], len[byte]); return; }
	uint32_t eb, ev;
	const uint32_t s = 257 + png_length_symbol(token, &eb, &ev), l = len[s];
	sink.put(code[s] | (ev << l), l + eb + 1);                                     /* and the distance code: one 0 bit */
}

PNG_HD uint32_t
png_token_bits(uint32_t byte, uint32_t token, const uint8_t *len)
{
	if (token == 1) return len[byte];
	uint32_t eb, ev;
	return len[257 + png_length_symbol(token, &eb, &ev)] + eb + 1;
}

/* ---- CRC-32 ---- */
struct PngCrcTable { uint32_t t[256]; };
constexpr PngCrcTable
png_make_crc()
{
	PngCrcTable c{};
	for (uint32_t n = 0; n < 256; n++) {
		uint32_t v = n;
		for (int k = 0; k < 8; k++) v = (v & 1u) ? (v >> 1) ^ PNG_POLY : v >> 1;
		c.t[n] = v;
	}
	return c;
}

/* a b mod the polynomial; bit 31 is x^0 */
PNG_HD constexpr uint32_t
png_gf_mul(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; i++) {
		if (a & (0x80000000u >> i)) p ^= b;
		b = (b >> 1) ^ ((b & 1u) ? PNG_POLY : 0u);
	}
	return p;
}

/* x^(8 2^k) for k = 0 .. 31: a register moved over n zero bytes is the register times x^(8 n) */
struct PngCrcPowers { uint32_t p[32]; };
constexpr PngCrcPowers
png_make_powers()
{
	PngCrcPowers x{};
	x.p[0] = 0x00800000u;
	for (int k = 1; k < 32; k++) x.p[k] = png_gf_mul(x.p[k - 1], x.p[k - 1]);
	return x;
}

/* the CRC register after "IDAT", from FFFFFFFF */
constexpr uint32_t
png_idat_register()
{
	const PngCrcTable c = png_make_crc();
	uint32_t r = 0xFFFFFFFFu;
	const char *s = "IDAT";
	for (int i = 0; i < 4; i++) r = c.t[(r ^ static_cast<uint8_t>(s[i])) & 255u] ^ (r >> 8);
	return r;
}

/* ---- sizes ---- */
inline uint32_t png_segment_bytes(uint32_t segment) { return (segment ? segment : MDEMOD_PNG_MAX_SEGMENT) * 1024u; }
inline uint32_t png_channels(uint32_t planes, uint32_t has_valid) { return planes + (has_valid ? 1u : 0u); }
inline uint64_t png_filtered_bytes(uint32_t width, uint32_t height, uint32_t channels) { return static_cast<uint64_t>(height) * (1ull + static_cast<uint64_t>(width) * channels); }
inline uint64_t png_segments(uint64_t n_bytes, uint32_t seg_bytes) { return (n_bytes + seg_bytes - 1) / seg_bytes; }
inline uint32_t png_slot_bytes(uint32_t seg_bytes) { return seg_bytes + 20u; }                 /* a chunk: len + 17 at most, in whole words */

/* the arguments of the entries: MDEMOD_OK, or MDEMOD_ERR_PARAM with the text noted */
int  png_check_picture(const char *who, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment);
int  png_check_bytes(const char *who, uint64_t n_bytes, uint32_t segment);
/* the file's bytes before the first segment into head[MDEMOD_PNG_HEAD] */
void png_head(uint32_t width, uint32_t height, uint32_t planes, uint32_t has_valid, uint8_t *head);

extern "C" {

/* ---- the host model: what the kernels of csrc/png.hip must compute, byte for byte (exported for the tests) ---- */

/* filtered[height (1 + width channels)] := the filtered stream of the picture and the mask (or NULL) */
int  mdemod_png_model_filter(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint8_t *filtered);
/* bytes[n_bytes] into the segments' IDAT chunks: *bytes_out := their number, always; written when they fit out_room, else
 * MDEMOD_ERR_OVERFLOW and nothing written.  stored (may be NULL) := the segments that took the stored fallback. */
int  mdemod_png_model_deflate(const uint8_t *bytes, uint64_t n_bytes, uint32_t segment, uint8_t *out, uint64_t out_room, uint64_t *bytes_out, uint64_t *stored);
/* the whole file, as mdemod_png_model_deflate gives its bytes */
int  mdemod_png_model_encode(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment,
                             uint8_t *out, uint64_t out_room, uint64_t *bytes_out);

}

#endif
