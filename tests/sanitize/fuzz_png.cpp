/*
 * fuzz_png.cpp — the host side of the PNG encoder (csrc/png_host.cpp) under ASan + UBSan (tests/test_png_sanitize.py).
 * Per case: a picture of a random size (1 x 1 .. 300 x 90), grey or colour, with a mask or without, noise, flat, a checkerboard or
 * noise inside a flat border, a filter and a segment size, now and then out of range, through the model's filter and its whole file;
 * or any bytes through its deflate stage.  out_room runs from 0 to the bound: too little is refused with the bytes needed and
 * nothing written.  Every buffer is exactly as long as the interface says and comes from the heap, so that one byte too far is a
 * report.  Every accepted stream is read back by the small inflater below (its own tables; stored and dynamic blocks, distance 1
 * only, as the header promises): every chunk's CRC, the chunk order, one final block at the very end, the Adler-32, and the bytes
 * that went in.  Prints one JSON line.
 * Usage: fuzz_png <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_png.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

extern "C" {
int  mdemod_png_model_filter(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint8_t *filtered);
int  mdemod_png_model_deflate(const uint8_t *bytes, uint64_t n_bytes, uint32_t segment, uint8_t *out, uint64_t out_room, uint64_t *bytes_out, uint64_t *stored);
int  mdemod_png_model_encode(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment,
                             uint8_t *out, uint64_t out_room, uint64_t *bytes_out);
}

static uint32_t
crc32_of(const uint8_t *p, size_t n)
{
	uint32_t r = 0xFFFFFFFFu;
	for (size_t i = 0; i < n; i++) {
		r ^= p[i];
		for (int k = 0; k < 8; k++) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1;
	}
	return r ^ 0xFFFFFFFFu;
}

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

/* ---- a small inflater: raw deflate, first bit lowest ---- */
struct Bits {
	const std::vector<uint8_t> &b;
	size_t pos = 0;
	explicit Bits(const std::vector<uint8_t> &bytes) : b(bytes) {}
	int bit() { if (pos >= 8 * b.size()) return -1; const int v = (b[pos >> 3] >> (pos & 7)) & 1; pos++; return v; }
	int bits(int n) { int v = 0; for (int i = 0; i < n; i++) { const int x = bit(); if (x < 0) return -1; v |= x << i; } return v; }
};

struct Code {
	int count[16] = { 0 };
	std::vector<int> symbol;
	/* from the lengths: 0 a complete code, 1 an incomplete one, -1 over-subscribed */
	int make(const int *len, int n)
	{
		for (int &c : count) c = 0;
		for (int i = 0; i < n; i++) count[len[i]]++;
		int left = 1;
		for (int l = 1; l < 16; l++) { left = 2 * left - count[l]; if (left < 0) return -1; }
		int offs[16] = { 0 };
		for (int l = 1; l < 15; l++) offs[l + 1] = offs[l] + count[l];
		symbol.assign(n, 0);
		for (int i = 0; i < n; i++) if (len[i]) symbol[offs[len[i]]++] = i;
		count[0] = 0;
		return left > 0;
	}
	int decode(Bits &in) const
	{
		int code = 0, first = 0, index = 0;
		for (int l = 1; l < 16; l++) {
			const int v = in.bit();
			if (v < 0) return -1;
			code |= v;
			if (code - count[l] < first) return symbol[index + (code - first)];
			index += count[l]; first += count[l]; first <<= 1; code <<= 1;
		}
		return -1;
	}
};

static const int LEN_BASE[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
static const int LEN_EXTRA[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
static const int CL_ORDER[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

struct Tally { uint64_t stored = 0, dynamic = 0, matches = 0, max_bits = 0; };

/* the whole stream back into out; false with a message on anything the header does not allow */
static bool
inflate(const std::vector<uint8_t> &z, std::vector<uint8_t> &out, Tally &t, long n)
{
	Bits in(z);
	out.clear();
	for (;;) {
		const int final = in.bit(), type = in.bits(2);
		if (final < 0 || type < 0) { FAIL("case %ld: the stream ends inside a block header", n); return false; }
		if (type == 0) {
			in.pos = (in.pos + 7) & ~size_t(7);
			const int len = in.bits(16), nlen = in.bits(16);
			if (len < 0 || nlen < 0 || (len ^ nlen) != 0xFFFF) { FAIL("case %ld: a stored block's lengths", n); return false; }
			if (in.pos / 8 + len > z.size()) { FAIL("case %ld: a stored block runs past the end", n); return false; }
			out.insert(out.end(), z.begin() + in.pos / 8, z.begin() + in.pos / 8 + len);
			in.pos += 8 * (size_t)len;
			t.stored += len != 0;
		} else if (type == 2) {
			const int hlit = in.bits(5) + 257, hdist = in.bits(5) + 1, hclen = in.bits(4) + 4;
			if (hlit > 286 || hdist != 1) { FAIL("case %ld: HLIT %d HDIST %d", n, hlit, hdist); return false; }
			int cl[19] = { 0 };
			for (int i = 0; i < hclen; i++) cl[CL_ORDER[i]] = in.bits(3);
			Code clcode;
			if (clcode.make(cl, 19) != 0) { FAIL("case %ld: the code-length code is not complete", n); return false; }
			int len[288] = { 0 };
			for (int i = 0; i < hlit + hdist;) {
				const int s = clcode.decode(in);
				if (s < 0) { FAIL("case %ld: a code-length symbol", n); return false; }
				if (s < 16) { len[i++] = s; continue; }
				int prev = 0, rep;
				if (s == 16) { if (!i) { FAIL("case %ld: a repeat with nothing before it", n); return false; } prev = len[i - 1]; rep = 3 + in.bits(2); }
				else rep = s == 17 ? 3 + in.bits(3) : 11 + in.bits(7);
				if (i + rep > hlit + hdist) { FAIL("case %ld: a repeat past the lengths", n); return false; }
				while (rep--) len[i++] = prev;
			}
			if (len[hlit] != 1) { FAIL("case %ld: the distance code's length is %d", n, len[hlit]); return false; }
			if (!len[256]) { FAIL("case %ld: no end-of-block code", n); return false; }
			Code ll;
			if (ll.make(len, hlit) != 0) { FAIL("case %ld: the literal/length code is not complete", n); return false; }
			for (int i = 0; i < hlit; i++) if ((uint64_t)len[i] > t.max_bits) t.max_bits = len[i];
			for (;;) {
				const int s = ll.decode(in);
				if (s < 0) { FAIL("case %ld: a literal/length symbol", n); return false; }
				if (s < 256) { out.push_back((uint8_t)s); continue; }
				if (s == 256) break;
				if (s > 285) { FAIL("case %ld: length symbol %d", n, s); return false; }
				const int length = LEN_BASE[s - 257] + in.bits(LEN_EXTRA[s - 257]);
				if (in.bit() != 0) { FAIL("case %ld: a distance code other than 0", n); return false; }
				if (out.empty()) { FAIL("case %ld: a match before any byte", n); return false; }
				out.insert(out.end(), (size_t)length, out.back());
				t.matches++;
			}
			t.dynamic++;
		} else { FAIL("case %ld: block type %d", n, type); return false; }
		if (final) break;
	}
	if ((in.pos + 7) / 8 != z.size()) { FAIL("case %ld: %zu bytes behind the final block", n, z.size() - (in.pos + 7) / 8); return false; }
	return true;
}

/* the chunks from `at` on: every CRC; the payloads of the IDATs appended to idat, their count to n_idat */
static bool
chunks(const uint8_t *f, uint64_t size, uint64_t at, std::vector<std::vector<uint8_t>> &idat, bool &iend, long n)
{
	iend = false;
	while (at < size) {
		if (at + 12 > size) { FAIL("case %ld: a chunk's frame runs past the end", n); return false; }
		const uint64_t len = be32(f + at);
		if (at + 12 + len > size) { FAIL("case %ld: a chunk's data runs past the end", n); return false; }
		if (crc32_of(f + at + 4, len + 4) != be32(f + at + 8 + len)) { FAIL("case %ld: the CRC of the chunk at %llu", n, (unsigned long long)at); return false; }
		if (!memcmp(f + at + 4, "IDAT", 4)) idat.emplace_back(f + at + 8, f + at + 8 + len);
		else if (!memcmp(f + at + 4, "IEND", 4) && len == 0 && at + 12 == size) iend = true;
		else { FAIL("case %ld: a chunk that is neither IDAT nor the last IEND", n); return false; }
		at += 12 + len;
	}
	return true;
}

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 100;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	long refused = 0, accepted = 0, pictures = 0, arrays = 0, short_rooms = 0, wild = 0, masks = 0;
	uint64_t stream_bytes = 0, in_bytes = 0;
	Tally t;
	std::vector<uint8_t> back, z;
	for (long n = 0; n < cases; n++) {
		uint32_t segment = static_cast<uint32_t>(rng() % 33);
		if (rng() % 3 == 0) segment = 1 + static_cast<uint32_t>(rng() % 2);
		if (rng() % 16 == 0) { segment = 33 + static_cast<uint32_t>(rng() % 1000); wild++; }
		const uint64_t sb = (segment ? segment : 32) * 1024ull;
		if (n % 2 == 0) {
			/* ---- a picture ---- */
			pictures++;
			uint32_t width = 1 + static_cast<uint32_t>(rng() % (rng() % 4 == 0 ? 300 : 40)), height = 1 + static_cast<uint32_t>(rng() % (rng() % 4 == 0 ? 90 : 30));
			uint32_t planes = rng() & 1 ? 1 : 3, filter = static_cast<uint32_t>(rng() % 6);
			if (rng() % 20 == 0) planes = static_cast<uint32_t>(rng() % 6);
			if (rng() % 20 == 0) filter = 6 + static_cast<uint32_t>(rng() % 1000);
			if (rng() % 30 == 0) width = rng() & 1 ? 0 : 8193;
			if (rng() % 30 == 0) height = rng() & 1 ? 0 : 16385;
			const bool masked = rng() % 2 == 0;
			const bool size_fine = (planes == 1 || planes == 3) && width >= 1 && width <= 8192 && height >= 1 && height <= 16384;
			const bool fine = size_fine && filter <= 5 && segment <= 32;
			const uint32_t pl = planes == 1 || planes == 3 ? planes : 1, w = width && width <= 8192 ? width : 8, h = height && height <= 16384 ? height : 8;
			const size_t px = static_cast<size_t>(w) * h, area = px * pl, ch = pl + masked, n_filtered = static_cast<size_t>(h) * (1 + w * ch);
			auto pic = exact<uint8_t>(area);
			auto valid = exact<uint8_t>(px);
			const int kind = static_cast<int>(rng() % 4);
			for (size_t k = 0; k < area; k++) {
				const size_t p = k / pl, x = p % w, y = p / w;
				const bool border = x < w / 5 || y < h / 5;
				pic[k] = kind == 0 ? static_cast<uint8_t>(rng()) : kind == 1 ? 77 : kind == 2 ? static_cast<uint8_t>(((x + y) & 1) * 255) : border ? 0 : static_cast<uint8_t>(100 + rng() % 9);
			}
			for (size_t k = 0; k < px; k++) valid[k] = rng() % 5 ? static_cast<uint8_t>(1 + rng() % 255) : 0;
			const uint8_t *va = masked ? valid.get() : nullptr;
			const uint64_t bound = mdemod_png_bound(width, height, planes, masked, segment);
			if ((bound != 0) != (size_fine && segment <= 32)) FAIL("case %ld: the bound is %llu", n, (unsigned long long)bound);
			auto filtered = exact<uint8_t>(n_filtered);
			const int rc0 = mdemod_png_model_filter(pic.get(), va, width, height, planes, filter, filtered.get());
			if ((rc0 == MDEMOD_OK) != (size_fine && filter <= 5)) FAIL("case %ld: the filter came back %d", n, rc0);
			const uint64_t room0 = bound ? bound : 1000;
			auto file = exact<uint8_t>(room0);
			uint64_t need = 0;
			const int rc = mdemod_png_model_encode(pic.get(), va, width, height, planes, filter, segment, file.get(), room0, &need);
			if ((rc == MDEMOD_OK) != fine) { FAIL("case %ld: %u x %u x %u filter %u segment %u came back %d", n, width, height, planes, filter, segment, rc); continue; }
			if (!fine) { if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: a refusal without its code or text", n); refused++; continue; }
			accepted++;
			masks += masked;
			stream_bytes += need; in_bytes += n_filtered;
			const uint64_t n_seg = (n_filtered + sb - 1) / sb;
			static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
			std::vector<std::vector<uint8_t>> idat;
			bool iend = false;
			if (need > bound || bound != MDEMOD_PNG_HEAD + MDEMOD_PNG_TAIL + n_filtered + MDEMOD_PNG_SEGMENT_OVERHEAD * n_seg || need < MDEMOD_PNG_HEAD + MDEMOD_PNG_TAIL ||
			    memcmp(file.get(), sig, 8) || be32(file.get() + 8) != 13 || memcmp(file.get() + 12, "IHDR", 4) || be32(file.get() + 16) != width || be32(file.get() + 20) != height ||
			    file[24] != 8 || file[25] != (planes == 3 ? 2 : 0) + (masked ? 4 : 0) || file[26] || file[27] || file[28] || crc32_of(file.get() + 12, 17) != be32(file.get() + 29))
				FAIL("case %ld: signature, IHDR or size (%llu of %llu)", n, (unsigned long long)need, (unsigned long long)bound);
			else if (chunks(file.get(), need, 33, idat, iend, n)) {
				if (!iend || idat.size() != n_seg + 2 || idat[0].size() != 2 || idat[0][0] != 0x78 || (idat[0][0] * 256 + idat[0][1]) % 31 || idat.back().size() != 4)
					FAIL("case %ld: %zu IDAT chunks for %llu segments, or the zlib header", n, idat.size(), (unsigned long long)n_seg);
				else {
					z.clear();
					for (size_t k = 1; k + 1 < idat.size(); k++) z.insert(z.end(), idat[k].begin(), idat[k].end());
					if (inflate(z, back, t, n)) {
						uint32_t a = 1, b = 0;
						for (uint8_t v : back) { a = (a + v) % 65521u; b = (b + a) % 65521u; }
						if (back.size() != n_filtered || memcmp(back.data(), filtered.get(), n_filtered)) FAIL("case %ld: the stream does not inflate to the filtered bytes", n);
						if (be32(idat.back().data()) != (b << 16 | a)) FAIL("case %ld: the Adler-32", n);
					}
				}
			}
			/* too little room: the bytes needed, and nothing written */
			const uint64_t rooms[3] = { 0, need - 1, rng() % need };
			for (uint64_t room : rooms) {
				auto small = exact<uint8_t>(room);
				memset(small.get(), 0xA5, room);
				uint64_t again = 0;
				const int rs = mdemod_png_model_encode(pic.get(), va, width, height, planes, filter, segment, room ? small.get() : nullptr, room, &again);
				bool clean = true;
				for (uint64_t k = 0; k < room; k++) clean = clean && small[k] == 0xA5;
				if (rs != MDEMOD_ERR_OVERFLOW || again != need || !clean) FAIL("case %ld: out_room %llu of %llu came back %d", n, (unsigned long long)room, (unsigned long long)need, rs);
				short_rooms++;
			}
			auto tight = exact<uint8_t>(need);
			uint64_t again = 0;
			if (mdemod_png_model_encode(pic.get(), va, width, height, planes, filter, segment, tight.get(), need, &again) != MDEMOD_OK || again != need || memcmp(tight.get(), file.get(), need))
				FAIL("case %ld: out_room exactly %llu", n, (unsigned long long)need);
		} else {
			/* ---- any bytes ---- */
			arrays++;
			const uint64_t n_bytes = rng() % 24 == 0 ? 0 : 1 + rng() % (rng() % 4 == 0 ? 70000 : 3000);
			auto data = exact<uint8_t>(n_bytes);
			const int kind = static_cast<int>(rng() % 5);
			uint8_t held = 0;
			for (uint64_t k = 0; k < n_bytes; k++) {
				const uint64_t x = rng();
				if (kind == 1 ? x % 300 == 0 : kind == 2 ? x % 3 == 0 : true) held = static_cast<uint8_t>(x >> 8);
				data[k] = kind == 0 ? static_cast<uint8_t>(x) : kind == 3 ? 0 : kind == 4 ? static_cast<uint8_t>(__builtin_ctzll(x | (1ull << 40))) : held;
			}
			const bool fine = segment <= 32 && n_bytes >= 1;
			const uint64_t bound = mdemod_png_deflate_bound(n_bytes, segment);
			if ((bound != 0) != fine) FAIL("case %ld: the deflate bound is %llu", n, (unsigned long long)bound);
			const uint64_t room0 = bound ? bound : 500;
			auto out = exact<uint8_t>(room0);
			uint64_t need = 0, stored = 0;
			const int rc = mdemod_png_model_deflate(data.get(), n_bytes, segment, out.get(), room0, &need, &stored);
			if ((rc == MDEMOD_OK) != fine) { FAIL("case %ld: %llu bytes, segment %u came back %d", n, (unsigned long long)n_bytes, segment, rc); continue; }
			if (!fine) { if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: a refusal without its code or text", n); refused++; continue; }
			accepted++;
			stream_bytes += need; in_bytes += n_bytes;
			const uint64_t n_seg = (n_bytes + sb - 1) / sb;
			std::vector<std::vector<uint8_t>> idat;
			bool iend = false;
			const uint64_t stored_before = t.stored;
			if (need > bound || bound != n_bytes + MDEMOD_PNG_SEGMENT_OVERHEAD * n_seg) FAIL("case %ld: %llu bytes, the bound is %llu", n, (unsigned long long)need, (unsigned long long)bound);
			else if (chunks(out.get(), need, 0, idat, iend, n)) {
				z.clear();
				for (const auto &c : idat) z.insert(z.end(), c.begin(), c.end());
				if (iend || idat.size() != n_seg) FAIL("case %ld: %zu chunks for %llu segments", n, idat.size(), (unsigned long long)n_seg);
				else if (inflate(z, back, t, n)) {
					if (back.size() != n_bytes || memcmp(back.data(), data.get(), n_bytes)) FAIL("case %ld: the chunks do not inflate to the bytes", n);
					if (t.stored - stored_before != stored) FAIL("case %ld: %llu stored segments read, %llu told", n, (unsigned long long)(t.stored - stored_before), (unsigned long long)stored);
				}
			}
			const uint64_t room = rng() % need;
			auto small = exact<uint8_t>(room);
			memset(small.get(), 0xA5, room);
			uint64_t again = 0;
			const int rs = mdemod_png_model_deflate(data.get(), n_bytes, segment, room ? small.get() : nullptr, room, &again, nullptr);
			bool clean = true;
			for (uint64_t k = 0; k < room; k++) clean = clean && small[k] == 0xA5;
			if (rs != MDEMOD_ERR_OVERFLOW || again != need || !clean) FAIL("case %ld: out_room %llu of %llu came back %d", n, (unsigned long long)room, (unsigned long long)need, rs);
			short_rooms++;
		}
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"bad\": %ld, \"refused\": %ld, \"accepted\": %ld, \"pictures\": %ld, \"arrays\": %ld, \"short_rooms\": %ld, \"wild_segments\": %ld, "
	       "\"masks\": %ld, \"stored\": %llu, \"dynamic\": %llu, \"matches\": %llu, \"max_bits\": %llu, \"bytes_in\": %llu, \"bytes\": %llu}\n", bad ? "false" : "true", cases, bad, refused,
	       accepted, pictures, arrays, short_rooms, wild, masks, (unsigned long long)t.stored, (unsigned long long)t.dynamic, (unsigned long long)t.matches,
	       (unsigned long long)t.max_bits, (unsigned long long)in_bytes, (unsigned long long)stream_bytes);
	return bad ? 1 : 0;
}
