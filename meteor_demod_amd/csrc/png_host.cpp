/*
 * png_host.cpp — host side of the PNG encoder (include/meteor_demod_amd_png.h): the argument checks, the sizes, the head of a file,
 * and the host model of the kernels of csrc/png.hip (mdemod_png_model_*: the rule of csrc/png_host.h as plain loops, one row, one run
 * and one bit after the other).  Free of the GPU runtime.
 */
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_host.h"
#include "encoder_host.h"

namespace {

constexpr PngCrcTable CRC = png_make_crc();

/* the bits of one segment, the first lowest */
struct BitWriter {
	std::vector<uint8_t> &out;
	uint64_t acc = 0;
	uint32_t cnt = 0;
	explicit BitWriter(std::vector<uint8_t> &o) : out(o) {}
	void put(uint32_t bits, uint32_t count)
	{
		acc |= static_cast<uint64_t>(bits) << cnt;
		cnt += count;
		while (cnt >= 8) { out.push_back(static_cast<uint8_t>(acc & 255u)); acc >>= 8; cnt -= 8; }
	}
	void flush() { if (cnt) put(0, 8 - cnt); }
};

uint32_t
crc_update(uint32_t r, const uint8_t *p, size_t n)
{
	for (size_t i = 0; i < n; i++) r = CRC.t[(r ^ p[i]) & 255u] ^ (r >> 8);
	return r;
}

void
put32(std::vector<uint8_t> &out, uint32_t v)
{
	for (int s = 24; s >= 0; s -= 8) out.push_back(static_cast<uint8_t>(v >> s));
}

/* a chunk of `type` around `data`, appended to out */
void
chunk(std::vector<uint8_t> &out, const char *type, const uint8_t *data, size_t n)
{
	put32(out, static_cast<uint32_t>(n));
	const size_t at = out.size();
	out.insert(out.end(), type, type + 4);
	if (n) out.insert(out.end(), data, data + n);
	put32(out, crc_update(0xFFFFFFFFu, out.data() + at, n + 4) ^ 0xFFFFFFFFu);
}

/* the lengths and codes of an alphabet of n symbols from its counts */
void
make_code(const uint32_t *count, uint32_t n, uint32_t limit, uint8_t *len, uint16_t *code)
{
	uint16_t order[PNG_LL_ROOM], up[2 * PNG_LL_ROOM];
	uint32_t w[2 * PNG_LL_ROOM], num[16], leaves = 0;
	for (uint32_t s = 0; s < n; s++)
		if (count[s]) order[leaves++] = static_cast<uint16_t>(s);
	std::sort(order, order + leaves, [&](uint16_t a, uint16_t b) { return png_before(count, a, b); });
	memset(len, 0, n);
	png_code_lengths(count, order, leaves, limit, len, w, up, num);
	/* RFC 1951 3.2.2, as it stands there; the kernels take png_code_of per symbol */
	uint32_t bl[17] = { 0 }, next[17] = { 0 }, c = 0;
	for (uint32_t s = 0; s < n; s++) bl[len[s]]++;
	bl[0] = 0;
	for (uint32_t l = 1; l <= 16; l++) { c = (c + bl[l - 1]) << 1; next[l] = c; }
	for (uint32_t s = 0; s < n; s++) {
		const uint32_t l = len[s];
		uint32_t v = l ? next[l]++ : 0, rev = 0;
		for (uint32_t b = 0; b < l; b++) rev |= ((v >> b) & 1u) << (l - 1 - b);
		code[s] = static_cast<uint16_t>(rev);
	}
}

/* f(byte, token) for every token of the segment, in order */
template <class F>
void
walk(const uint8_t *p, uint32_t n, F f)
{
	for (uint32_t s = 0; s < n;) {
		uint32_t e = s + 1;
		while (e < n && p[e] == p[s]) e++;
		for (uint32_t k = 0; k < e - s; k++) {
			const uint32_t t = png_token(k, e - s);
			if (t) f(p[s], t);
		}
		s = e;
	}
}

/* one segment's deflate bytes; returns whether it is stored */
bool
model_segment(const uint8_t *p, uint32_t n, bool last, std::vector<uint8_t> &out)
{
	uint32_t count[PNG_LL_ROOM] = { 0 }, clcount[PNG_CL] = { 0 };
	uint8_t len[PNG_LL_ROOM + 1], cllen[PNG_CL];
	uint16_t code[PNG_LL_ROOM], clcode[PNG_CL], tok[PNG_LL_ROOM];
	walk(p, n, [&](uint32_t byte, uint32_t t) {
		uint32_t eb, ev;
		count[t == 1 ? byte : 257 + png_length_symbol(t, &eb, &ev)]++;
	});
	count[PNG_EOB]++;
	make_code(count, PNG_LL, 15, len, code);
	uint32_t hlit = PNG_LL;
	while (hlit > 257 && !len[hlit - 1]) hlit--;
	len[hlit] = 1;                                                                 /* the distance code */
	const uint32_t n_tok = png_rle(len, hlit + 1, tok, clcount);
	make_code(clcount, PNG_CL, 7, cllen, clcode);
	uint64_t bits = png_header_bits(tok, n_tok, cllen) + len[PNG_EOB] + 3;
	walk(p, n, [&](uint32_t byte, uint32_t t) { bits += png_token_bits(byte, t, len); });
	const uint64_t dynamic = (bits + 7) / 8 + 4;
	if (dynamic > static_cast<uint64_t>(n) + 5) {
		out.push_back(last ? 1 : 0);
		out.push_back(static_cast<uint8_t>(n & 255u)); out.push_back(static_cast<uint8_t>(n >> 8));
		out.push_back(static_cast<uint8_t>(~n & 255u)); out.push_back(static_cast<uint8_t>((~n >> 8) & 255u));
		out.insert(out.end(), p, p + n);
		return true;
	}
	BitWriter w(out);
	png_put_header(w, hlit, tok, n_tok, cllen, clcode);
	walk(p, n, [&](uint32_t byte, uint32_t t) { png_put_token(w, byte, t, len, code); });
	w.put(code[PNG_EOB], len[PNG_EOB]);
	w.put(last ? 1 : 0, 3);                                                        /* the empty stored block */
	w.flush();
	out.push_back(0); out.push_back(0); out.push_back(0xFF); out.push_back(0xFF);
	return false;
}

/* the segments' chunks, appended to out; returns the stored ones */
uint64_t
model_chunks(const uint8_t *bytes, uint64_t n_bytes, uint32_t seg_bytes, std::vector<uint8_t> &out)
{
	uint64_t stored = 0;
	std::vector<uint8_t> z;
	for (uint64_t at = 0; at < n_bytes; at += seg_bytes) {
		const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(seg_bytes, n_bytes - at));
		z.clear();
		stored += model_segment(bytes + at, n, at + n == n_bytes, z);
		chunk(out, "IDAT", z.data(), z.size());
	}
	return stored;
}

void
model_filter(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint8_t *filtered)
{
	const uint32_t ch = png_channels(planes, valid != nullptr), row = width * ch;
	std::vector<uint8_t> cur(row), prev(row, 0);
	for (uint32_t y = 0; y < height; y++) {
		for (uint32_t x = 0; x < width; x++) {
			for (uint32_t c = 0; c < planes; c++) cur[x * ch + c] = picture[(static_cast<size_t>(y) * width + x) * planes + c];
			if (valid) cur[x * ch + planes] = valid[static_cast<size_t>(y) * width + x] ? 255 : 0;
		}
		auto at = [&](uint32_t f, uint32_t i) {
			const uint32_t a = i >= ch ? cur[i - ch] : 0u, c = i >= ch ? prev[i - ch] : 0u;
			return png_filter_byte(f, cur[i], a, prev[i], c);
		};
		uint32_t f = filter;
		if (filter == MDEMOD_PNG_FILTER_ADAPT) {
			uint32_t sum[5] = { 0, 0, 0, 0, 0 };
			for (uint32_t g = 0; g < 5; g++)
				for (uint32_t i = 0; i < row; i++) sum[g] += png_cost(at(g, i));
			f = png_choose(sum);
		}
		uint8_t *to = filtered + static_cast<size_t>(y) * (1 + row);
		to[0] = static_cast<uint8_t>(f);
		for (uint32_t i = 0; i < row; i++) to[1 + i] = static_cast<uint8_t>(at(f, i));
		cur.swap(prev);
	}
}

} /* namespace */

int
png_check_picture(const char *who, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment)
{
	if (planes != 1 && planes != 3) REFUSE("%s: planes must be 1 or 3, not %u", who, planes);
	if (width < 1 || width > MDEMOD_PNG_MAX_WIDTH) REFUSE("%s: width %u is outside 1 .. %d", who, width, MDEMOD_PNG_MAX_WIDTH);
	if (height < 1 || height > MDEMOD_PNG_MAX_HEIGHT) REFUSE("%s: height %u is outside 1 .. %d", who, height, MDEMOD_PNG_MAX_HEIGHT);
	if (filter > MDEMOD_PNG_FILTER_ADAPT) REFUSE("%s: filter %u is outside 0 .. %d", who, filter, MDEMOD_PNG_FILTER_ADAPT);
	if (segment > MDEMOD_PNG_MAX_SEGMENT) REFUSE("%s: segment %u KiB is outside 0 .. %d", who, segment, MDEMOD_PNG_MAX_SEGMENT);
	return MDEMOD_OK;
}

int
png_check_bytes(const char *who, uint64_t n_bytes, uint32_t segment)
{
	if (n_bytes < 1 || n_bytes > MDEMOD_PNG_MAX_BYTES) REFUSE("%s: %llu bytes are outside 1 .. 2^30", who, static_cast<unsigned long long>(n_bytes));
	if (segment > MDEMOD_PNG_MAX_SEGMENT) REFUSE("%s: segment %u KiB is outside 0 .. %d", who, segment, MDEMOD_PNG_MAX_SEGMENT);
	return MDEMOD_OK;
}

void
png_head(uint32_t width, uint32_t height, uint32_t planes, uint32_t has_valid, uint8_t *head)
{
	static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
	std::vector<uint8_t> out(sig, sig + 8);
	std::vector<uint8_t> ihdr;
	put32(ihdr, width); put32(ihdr, height);
	ihdr.push_back(8);
	ihdr.push_back(static_cast<uint8_t>((planes == 3 ? 2 : 0) + (has_valid ? 4 : 0)));
	ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
	chunk(out, "IHDR", ihdr.data(), ihdr.size());
	const uint8_t zlib[2] = { 0x78, 0x01 };
	chunk(out, "IDAT", zlib, 2);
	memcpy(head, out.data(), MDEMOD_PNG_HEAD);
}

extern "C" {

uint64_t
mdemod_png_deflate_bound(uint64_t n_bytes, uint32_t segment)
{
	if (n_bytes < 1 || n_bytes > MDEMOD_PNG_MAX_BYTES || segment > MDEMOD_PNG_MAX_SEGMENT) return 0;
	return n_bytes + MDEMOD_PNG_SEGMENT_OVERHEAD * png_segments(n_bytes, png_segment_bytes(segment));
}

uint64_t
mdemod_png_bound(uint32_t width, uint32_t height, uint32_t planes, uint32_t has_valid, uint32_t segment)
{
	if (width < 1 || width > MDEMOD_PNG_MAX_WIDTH || height < 1 || height > MDEMOD_PNG_MAX_HEIGHT || (planes != 1 && planes != 3)) return 0;
	const uint64_t e = mdemod_png_deflate_bound(png_filtered_bytes(width, height, png_channels(planes, has_valid)), segment);
	return e ? e + MDEMOD_PNG_HEAD + MDEMOD_PNG_TAIL : 0;
}

uint64_t
mdemod_png_deflate_workspace(uint64_t n_bytes, uint32_t segment)
{
	if (!mdemod_png_deflate_bound(n_bytes, segment)) return 0;
	const uint32_t sb = png_segment_bytes(segment);
	const uint64_t n_seg = png_segments(n_bytes, sb);
	return n_seg * png_slot_bytes(sb) + (n_seg + 1) * 8 + n_seg * 12 + 16;        /* the chunks, the offsets, the lengths and the Adler sums */
}

uint64_t
mdemod_png_workspace(uint32_t width, uint32_t height, uint32_t planes, uint32_t has_valid, uint32_t segment)
{
	if (!mdemod_png_bound(width, height, planes, has_valid, segment)) return 0;
	const uint64_t n = png_filtered_bytes(width, height, png_channels(planes, has_valid));
	return ((n + 15) & ~15ull) + mdemod_png_deflate_workspace(n, segment);
}

void mdemod_png_free(uint8_t *file) { free(file); }

int
mdemod_png_model_filter(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint8_t *filtered)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_png_model_filter";
	const int rc = png_check_picture(who, width, height, planes, filter, 0);
	if (rc) return rc;
	if (!picture || !filtered) REFUSE("%s: the picture and the filtered stream are needed", who);
	model_filter(picture, valid, width, height, planes, filter, filtered);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_png_model_deflate(const uint8_t *bytes, uint64_t n_bytes, uint32_t segment, uint8_t *out, uint64_t out_room, uint64_t *bytes_out, uint64_t *stored)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_png_model_deflate";
	const int rc = png_check_bytes(who, n_bytes, segment);
	if (rc) return rc;
	if (!bytes || (!out && out_room)) REFUSE("%s: the bytes and the output are needed", who);
	std::vector<uint8_t> file;
	const uint64_t s = model_chunks(bytes, n_bytes, png_segment_bytes(segment), file);
	if (stored) *stored = s;
	return enc_give(who, file, out, out_room, bytes_out);
} MDEMOD_API_CATCH

int
mdemod_png_model_encode(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment, uint8_t *out,
                        uint64_t out_room, uint64_t *bytes_out)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_png_model_encode";
	const int rc = png_check_picture(who, width, height, planes, filter, segment);
	if (rc) return rc;
	if (!picture || (!out && out_room)) REFUSE("%s: the picture and the output are needed", who);
	const uint64_t n = png_filtered_bytes(width, height, png_channels(planes, valid != nullptr));
	std::vector<uint8_t> filtered(n);
	model_filter(picture, valid, width, height, planes, filter, filtered.data());
	std::vector<uint8_t> file(MDEMOD_PNG_HEAD);
	png_head(width, height, planes, valid != nullptr, file.data());
	model_chunks(filtered.data(), n, png_segment_bytes(segment), file);
	uint32_t a = 1, b = 0;
	for (uint64_t i = 0; i < n; i++) { a = (a + filtered[i]) % PNG_ADLER; b = (b + a) % PNG_ADLER; }
	uint8_t adler[4] = { static_cast<uint8_t>(b >> 8), static_cast<uint8_t>(b), static_cast<uint8_t>(a >> 8), static_cast<uint8_t>(a) };
	chunk(file, "IDAT", adler, 4);
	chunk(file, "IEND", nullptr, 0);
	return enc_give(who, file, out, out_room, bytes_out);
} MDEMOD_API_CATCH

} /* extern "C" */
