/*
 * fuzz_jpeg.cpp — the host side of the JPEG encoder (csrc/jpeg_host.cpp) under ASan + UBSan (tests/test_jpeg_sanitize.py).
 * Per case: a picture of a random size (1 x 1 .. 300 x 90), grey or colour, noise, flat or a checkerboard of period 1, a quality and a
 * restart interval, now and then out of range, through the model's coefficients and its whole file; and a coefficient array of any
 * int16 values through its entropy coder.  out_room runs from 0 to the bound: too little is refused with the bytes needed and
 * nothing written.  Every buffer is exactly as long as the interface says and comes from the heap, so that one byte too far is a
 * report.  Every accepted stream is parsed back by the small decoder below: the head is the one asked for, every code is one of the
 * table, every interval holds its MCUs and ends in 1-bits, and the coefficients are those that went in, clamped.  Prints one JSON line.
 * Usage: fuzz_jpeg <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_jpeg.h"
#include "../../meteor_demod_amd/csrc/jpeg_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

static const JpegCodes CODES = jpeg_make_codes();
/* code | length << 16 -> symbol: [0] DC, [1] AC of the luminance, [2], [3] of the chrominance */
static std::map<uint32_t, int> TABLE[4];

static void
make_tables()
{
	for (int t = 0; t < 2; t++) {
		for (int s = 0; s < 12; s++) TABLE[2 * t][CODES.dc[t][s]] = s;
		for (int s = 0; s < 256; s++) if (CODES.ac[t][s]) TABLE[2 * t + 1][CODES.ac[t][s]] = s;
	}
}

struct Reader {
	const std::vector<uint8_t> &b;
	size_t pos = 0;                               /* in bits */
	explicit Reader(const std::vector<uint8_t> &bytes) : b(bytes) {}
	int bit() { if (pos >= 8 * b.size()) return -1; const int v = (b[pos >> 3] >> (7 - (pos & 7))) & 1; pos++; return v; }
	/* one code of table[n]: the symbol, or -1 */
	int symbol(const std::map<uint32_t, int> &table)
	{
		uint32_t code = 0;
		for (uint32_t len = 1; len <= 16; len++) {
			const int v = bit();
			if (v < 0) return -1;
			code = (code << 1) | static_cast<uint32_t>(v);
			const auto hit = table.find(code | (len << 16));
			if (hit != table.end()) return hit->second;
		}
		return -1;
	}
	bool value(int size, int &out)
	{
		int v = 0;
		for (int k = 0; k < size; k++) { const int x = bit(); if (x < 0) return false; v = (v << 1) | x; }
		out = size && v < (1 << (size - 1)) ? v - (1 << size) + 1 : v;
		return true;
	}
};

/* the segments and the markers between them back into coefficients; false and a message when they are no such stream */
static bool
parse_segments(const uint8_t *p, size_t n, uint64_t n_mcus, uint32_t planes, uint32_t ri, std::vector<int> &coef)
{
	coef.assign(n_mcus * planes * 64, 0);
	const uint64_t n_seg = (n_mcus + ri - 1) / ri;
	size_t at = 0;
	for (uint64_t s = 0; s < n_seg; s++) {
		std::vector<uint8_t> bytes;
		for (;;) {
			if (at == n) { if (s + 1 != n_seg) { FAIL("the stream ends in interval %llu of %llu", (unsigned long long)s, (unsigned long long)n_seg); return false; } break; }
			if (p[at] != 0xFF) { bytes.push_back(p[at++]); continue; }
			if (at + 1 == n) { FAIL("a lone FF at the end"); return false; }
			if (p[at + 1] == 0) { bytes.push_back(0xFF); at += 2; continue; }
			if (p[at + 1] != 0xD0 + (s & 7) || s + 1 == n_seg) { FAIL("marker FF %02X behind interval %llu", p[at + 1], (unsigned long long)s); return false; }
			at += 2;
			break;
		}
		Reader r(bytes);
		int pred[3] = { 0, 0, 0 };
		const uint64_t end = (s + 1) * ri < n_mcus ? (s + 1) * ri : n_mcus;
		for (uint64_t m = s * ri; m < end; m++)
			for (uint32_t c = 0; c < planes; c++) {
				int *blk = coef.data() + (m * planes + c) * 64, v = 0;
				const int size = r.symbol(TABLE[c ? 2 : 0]);
				if (size < 0 || !r.value(size, v)) { FAIL("no DC value in MCU %llu", (unsigned long long)m); return false; }
				blk[0] = pred[c] += v;
				for (int k = 1; k < 64;) {
					const int rs = r.symbol(TABLE[c ? 3 : 1]);
					if (rs < 0) { FAIL("no AC code in MCU %llu at %d", (unsigned long long)m, k); return false; }
					if (rs == 0) break;
					if (rs == 0xF0) { k += 16; if (k > 63) { FAIL("a ZRL past the block"); return false; } continue; }
					k += rs >> 4;
					if ((rs & 15) == 0 || (rs & 15) > 10 || k > 63 || !r.value(rs & 15, v)) { FAIL("a bad AC symbol %02X at %d", rs, k); return false; }
					blk[k++] = v;
				}
			}
		const size_t left = 8 * bytes.size() - r.pos;
		if (left >= 8) { FAIL("%zu bits behind interval %llu", left, (unsigned long long)s); return false; }
		for (size_t k = 0; k < left; k++) if (r.bit() != 1) { FAIL("padding of interval %llu is not 1-bits", (unsigned long long)s); return false; }
	}
	if (at != n) { FAIL("%zu bytes behind the last interval", n - at); return false; }
	return true;
}

static int clamp_level(int v, bool dc) { const int low = dc ? -1024 : -1023; return v < low ? low : v > 1023 ? 1023 : v; }

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 100;
	make_tables();
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	long refused = 0, accepted = 0, short_rooms = 0, pictures = 0, arrays = 0, ri_wild = 0;
	unsigned long long blocks = 0, stream_bytes = 0, stuffed = 0;
	for (long n = 0; n < cases; n++) {
		const uint32_t planes = rng() % 16 == 0 ? static_cast<uint32_t>(rng() % 5) : (rng() & 1 ? 3 : 1);
		uint32_t ri = static_cast<uint32_t>(rng() % 65);
		if (rng() % 16 == 0) { ri = 65 + static_cast<uint32_t>(rng() % 1000); ri_wild++; }
		const bool fine_common = (planes == 1 || planes == 3) && ri <= 64;
		const uint32_t step = ri ? ri : MDEMOD_JPEG_RESTART;
		std::vector<int> back;
		if (n % 2 == 0) {
			/* ---- a picture ---- */
			pictures++;
			uint32_t width = 1 + static_cast<uint32_t>(rng() % (rng() % 4 == 0 ? 300 : 40)), height = 1 + static_cast<uint32_t>(rng() % (rng() % 4 == 0 ? 90 : 30));
			uint32_t quality = 1 + static_cast<uint32_t>(rng() % 100);
			if (rng() % 20 == 0) quality = rng() & 1 ? 0 : 101 + static_cast<uint32_t>(rng() % 1000);
			if (rng() % 30 == 0) width = rng() & 1 ? 0 : 8193;
			if (rng() % 30 == 0) height = rng() & 1 ? 0 : 16385;
			const bool fine = fine_common && quality >= 1 && quality <= 100 && width >= 1 && width <= 8192 && height >= 1 && height <= 16384;
			const uint32_t pl = planes ? planes : 1, w = width && width <= 8192 ? width : 8, h = height && height <= 16384 ? height : 8;
			const size_t area = static_cast<size_t>(w) * h * pl;
			auto pic = exact<uint8_t>(area);
			const int kind = static_cast<int>(rng() % 3);
			for (size_t k = 0; k < area; k++) {
				const size_t px = k / pl;
				pic[k] = kind == 0 ? static_cast<uint8_t>(rng()) : kind == 1 ? 77 : static_cast<uint8_t>(((px % w + px / w) & 1) * 255);
			}
			const uint64_t n_mcus = jpeg_mcus(w, h), bound = mdemod_jpeg_bound(width, height, planes, ri);
			if ((bound != 0) != (fine_common && width >= 1 && width <= 8192 && height >= 1 && height <= 16384)) FAIL("case %ld: the bound is %llu", n, (unsigned long long)bound);
			auto coef = exact<int16_t>(n_mcus * pl * 64);
			const int rc0 = mdemod_jpeg_model_coefficients(pic.get(), width, height, planes, quality, coef.get());
			const bool fine0 = (planes == 1 || planes == 3) && quality >= 1 && quality <= 100 && width >= 1 && width <= 8192 && height >= 1 && height <= 16384;
			if ((rc0 == MDEMOD_OK) != fine0) FAIL("case %ld: the coefficients came back %d", n, rc0);
			const uint64_t room0 = bound ? bound : 1000;
			auto file = exact<uint8_t>(room0);
			uint64_t need = 0;
			const int rc = mdemod_jpeg_model_encode(pic.get(), width, height, planes, quality, ri, file.get(), room0, &need);
			if ((rc == MDEMOD_OK) != fine) { FAIL("case %ld: %u x %u x %u quality %u interval %u came back %d", n, width, height, planes, quality, ri, rc); continue; }
			if (!fine) { if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: a refusal without its code or text", n); refused++; continue; }
			accepted++;
			blocks += n_mcus * planes; stream_bytes += need;
			uint8_t head[JPEG_HEAD_ROOM];
			const uint32_t head_n = jpeg_head(width, height, planes, quality, ri, head);
			if (head_n != (planes == 3 ? MDEMOD_JPEG_HEAD_COLOUR : MDEMOD_JPEG_HEAD_GREY) || need < head_n + 2 || need > bound || memcmp(file.get(), head, head_n) ||
			    file[need - 2] != 0xFF || file[need - 1] != 0xD9)
				FAIL("case %ld: head, EOI or size (%llu of %llu)", n, (unsigned long long)need, (unsigned long long)bound);
			else if (parse_segments(file.get() + head_n, need - head_n - 2, n_mcus, planes, step, back)) {
				for (size_t k = 0; k < back.size(); k++)
					if (back[k] != coef[k]) { FAIL("case %ld: coefficient %zu reads %d, was %d", n, k, back[k], coef[k]); break; }
				for (uint64_t k = head_n; k + 1 < need; k++) stuffed += file[k] == 0xFF && file[k + 1] == 0;
			}
			/* too little room: the bytes needed, and nothing written */
			const uint64_t rooms[3] = { 0, need - 1, rng() % need };
			for (uint64_t room : rooms) {
				auto small = exact<uint8_t>(room);
				memset(small.get(), 0xA5, room);
				uint64_t again = 0;
				const int rs = mdemod_jpeg_model_encode(pic.get(), width, height, planes, quality, ri, room ? small.get() : nullptr, room, &again);
				bool clean = true;
				for (uint64_t k = 0; k < room; k++) clean = clean && small[k] == 0xA5;
				if (rs != MDEMOD_ERR_OVERFLOW || again != need || !clean) FAIL("case %ld: out_room %llu of %llu came back %d", n, (unsigned long long)room, (unsigned long long)need, rs);
				short_rooms++;
			}
			auto tight = exact<uint8_t>(need);
			uint64_t again = 0;
			if (mdemod_jpeg_model_encode(pic.get(), width, height, planes, quality, ri, tight.get(), need, &again) != MDEMOD_OK || again != need || memcmp(tight.get(), file.get(), need))
				FAIL("case %ld: out_room exactly %llu", n, (unsigned long long)need);
		} else {
			/* ---- any coefficients ---- */
			arrays++;
			const uint64_t n_mcus = rng() % 24 == 0 ? 0 : 1 + rng() % 100;
			const uint32_t pl = planes ? planes : 1;
			const size_t count = static_cast<size_t>(n_mcus) * pl * 64;
			auto coef = exact<int16_t>(count);
			const int kind = static_cast<int>(rng() % 4);
			for (size_t k = 0; k < count; k++) {
				const uint64_t x = rng();
				coef[k] = kind == 0 ? static_cast<int16_t>(x) : kind == 1 ? (x % 7 == 0 ? static_cast<int16_t>(x >> 8) : 0) : kind == 2 ? (x & 1 ? 32767 : -32768)
				                                                                                                                          : static_cast<int16_t>(static_cast<int>((x >> 8) % 2049) - 1024);
			}
			const bool fine = fine_common && n_mcus >= 1;
			const uint64_t bound = mdemod_jpeg_entropy_bound(n_mcus, planes, ri);
			if ((bound != 0) != fine) FAIL("case %ld: the entropy bound is %llu", n, (unsigned long long)bound);
			const uint64_t room0 = bound ? bound : 500;
			auto out = exact<uint8_t>(room0);
			uint64_t need = 0;
			const int rc = mdemod_jpeg_model_entropy(coef.get(), n_mcus, planes, ri, out.get(), room0, &need);
			if ((rc == MDEMOD_OK) != fine) { FAIL("case %ld: %llu MCUs x %u interval %u came back %d", n, (unsigned long long)n_mcus, planes, ri, rc); continue; }
			if (!fine) { if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: a refusal without its code or text", n); refused++; continue; }
			accepted++;
			blocks += n_mcus * planes; stream_bytes += need;
			if (need > bound) FAIL("case %ld: %llu bytes, the bound is %llu", n, (unsigned long long)need, (unsigned long long)bound);
			else if (parse_segments(out.get(), need, n_mcus, planes, step, back)) {
				for (size_t k = 0; k < back.size(); k++)
					if (back[k] != clamp_level(coef[k], k % 64 == 0)) { FAIL("case %ld: coefficient %zu reads %d, was %d", n, k, back[k], coef[k]); break; }
				for (uint64_t k = 0; k + 1 < need; k++) stuffed += out[k] == 0xFF && out[k + 1] == 0;
			}
			const uint64_t room = rng() % need;
			auto small = exact<uint8_t>(room);
			memset(small.get(), 0xA5, room);
			uint64_t again = 0;
			const int rs = mdemod_jpeg_model_entropy(coef.get(), n_mcus, planes, ri, room ? small.get() : nullptr, room, &again);
			bool clean = true;
			for (uint64_t k = 0; k < room; k++) clean = clean && small[k] == 0xA5;
			if (rs != MDEMOD_ERR_OVERFLOW || again != need || !clean) FAIL("case %ld: out_room %llu of %llu came back %d", n, (unsigned long long)room, (unsigned long long)need, rs);
			short_rooms++;
		}
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"bad\": %ld, \"refused\": %ld, \"accepted\": %ld, \"pictures\": %ld, \"arrays\": %ld, \"short_rooms\": %ld, \"wild_intervals\": %ld, "
	       "\"blocks\": %llu, \"bytes\": %llu, \"stuffed\": %llu}\n", bad ? "false" : "true", cases, bad, refused, accepted, pictures, arrays, short_rooms, ri_wild, blocks,
	       stream_bytes, stuffed);
	return bad ? 1 : 0;
}
