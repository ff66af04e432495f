/*
 * fuzz_picture.cpp — the host side of the picture layer (csrc/picture_host.cpp) under ASan + UBSan (tests/test_picture_sanitize.py):
 * random options (some out of range: refused with MDEMOD_ERR_PARAM and a text), the column map into a buffer of exactly W entries,
 * random histograms through the table, pictures of 0 .. 5 strip rows under random masks through the model's histogram and render
 * (grey and colour, random selections, sometimes a map with entries beyond the line), and the whole-picture entry's model path in
 * pieces of 0 .. 6 rows against one batch.  Every buffer is exactly as long as the interface says and comes from the heap, so that
 * one byte too far is a report.  What comes back is checked against the rules that hold for any input.  Prints one JSON line.
 * Usage: fuzz_picture <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "../../include/meteor_demod_amd_picture.h"
#include "../../meteor_demod_amd/csrc/picture_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 200;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	long refused = 0, empty = 0, grey = 0, colour = 0, stretched = 0, identity = 0, pieces = 0;
	std::set<uint32_t> widths;
	for (long i = 0; i < cases; i++) {
		mdemod_picture_opts o;
		mdemod_picture_default_opts(&o);
		if (rng() & 1) {
			o.altitude_km = 300.0 + static_cast<double>(rng() % 170001) / 100.0;
			o.scan_deg = 1.0 + static_cast<double>(rng() % 12901) / 100.0;
		}
		o.rectify = rng() % 4 != 0;
		o.stretch = rng() % 4 != 0;
		o.clip_low = static_cast<uint32_t>(rng() % 500);
		o.clip_high = static_cast<uint32_t>(rng() % 500);
		o.piece_rows = static_cast<uint32_t>(rng() % 7);
		bool broken = false;
		if (rng() % 10 == 0) {
			broken = true;
			switch (rng() % 5) {
			case 0: o.altitude_km = rng() & 1 ? 299.0 : 2001.0; break;
			case 1: o.scan_deg = rng() & 1 ? 0.5 : 131.0; break;
			case 2: o.clip_low = 500 + static_cast<uint32_t>(rng() % 1000); break;
			case 3: o.clip_high = 500 + static_cast<uint32_t>(rng() % 1000); break;
			default: o.piece_rows = 65537 + static_cast<uint32_t>(rng() % 1000); break;
			}
		}
		uint32_t width = 0;
		int rc = mdemod_picture_column_map(&o, nullptr, 0, &width);
		const uint32_t rows = static_cast<uint32_t>(rng() % 6), planes = rng() & 1 ? 3 : 1;
		uint32_t select[3] = { static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3) };
		/* ---- the pictures and masks, each exactly as long as its rows ---- */
		std::unique_ptr<uint8_t[]> img[3], fil[3];
		const uint8_t *image[3], *filled[3];
		const int mask_kind = static_cast<int>(rng() % 4);
		for (int s = 0; s < 3; s++) {
			img[s] = exact<uint8_t>(rows * PIC_LINE_BYTES);
			fil[s] = exact<uint8_t>(static_cast<size_t>(rows) * PIC_CELLS);
			for (size_t k = 0; k < rows * PIC_LINE_BYTES; k++) img[s][k] = static_cast<uint8_t>(rng());
			for (size_t k = 0; k < static_cast<size_t>(rows) * PIC_CELLS; k++)
				fil[s][k] = mask_kind == 0 ? 1 : mask_kind == 1 ? 0 : mask_kind == 2 ? static_cast<uint8_t>((k + s) & 1) : static_cast<uint8_t>(rng() & 1 ? rng() : 0);
			image[s] = img[s].get();
			filled[s] = fil[s].get();
		}
		if (!rc && !broken && o.rectify == 0 && width != 1568) FAIL("case %ld: the identity map is %u wide", i, width);
		if (rc == MDEMOD_OK && broken) FAIL("case %ld: options out of range were accepted", i);
		if (rc != MDEMOD_OK) {
			/* refused (out of range, or a scan whose edge misses the Earth): a text, and the whole-picture entry refuses them too */
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: the map gave rc %d, text '%s'", i, rc, mdemod_last_error());
			mdemod_picture_result res;
			rc = mdemod_picture_model_host(&o, image, filled, rows, select, planes, &res);
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: the host entry took refused options (rc %d)", i, rc);
			refused++;
			continue;
		}
		/* ---- the map: exactly W entries ---- */
		if (width < 4 || width > MDEMOD_PICTURE_MAX_WIDTH || width % 4) { FAIL("case %ld: width %u", i, width); continue; }
		widths.insert(width);
		auto map = exact<uint32_t>(width);
		uint32_t again = 0;
		rc = mdemod_picture_column_map(&o, map.get(), width, &again);
		if (rc != MDEMOD_OK || again != width) { FAIL("case %ld: the map with room gave rc %d, width %u of %u", i, rc, again, width); continue; }
		for (uint32_t j = 0; j < width; j++) {
			if (map[j] > 1567u * 256u || map[j] + map[width - 1 - j] != 1567u * 256u || (j && map[j] < map[j - 1])) { FAIL("case %ld: map[%u] = %u breaks the rules", i, j, map[j]); break; }
		}
		if (width > 4) {
			auto few = exact<uint32_t>(width - 4);
			rc = mdemod_picture_column_map(&o, few.get(), width - 4, &again);
			if (rc != MDEMOD_ERR_PARAM || again != width) FAIL("case %ld: a map without room gave rc %d", i, rc);
		}
		/* ---- the model's histogram, the tables ---- */
		auto hist = exact<uint32_t>(3 * 256);
		rc = mdemod_picture_model_histogram(image, filled, rows, hist.get());
		if (rc != MDEMOD_OK) { FAIL("case %ld: the histogram refused: %s", i, mdemod_last_error()); continue; }
		for (int s = 0; s < 3; s++) {
			uint64_t sum = 0, cells = 0;
			for (int v = 0; v < 256; v++) sum += hist[256 * s + v];
			for (size_t k = 0; k < static_cast<size_t>(rows) * PIC_CELLS; k++) cells += fil[s][k] != 0;
			if (sum != cells * 8 * PIC_CELL_W) FAIL("case %ld: slot %d counts %llu pixels in %llu cells", i, s, (unsigned long long)sum, (unsigned long long)cells);
		}
		auto lut = exact<uint8_t>(256 * planes);
		for (uint32_t p = 0; p < planes; p++) {
			auto h = exact<uint32_t>(256);
			const int kind = static_cast<int>(rng() % 4);
			for (int v = 0; v < 256; v++)
				h[v] = kind == 0 ? hist[256 * select[p] + v] : kind == 1 ? 0u : kind == 2 ? (v == 99 ? 5u : 0u) : static_cast<uint32_t>(rng() & 1 ? rng() : 0);
			uint32_t lim[2] = { 9, 9 };
			rc = mdemod_picture_lut(h.get(), o.clip_low, o.clip_high, lut.get() + 256 * p, lim);
			if (rc != MDEMOD_OK || lim[0] > lim[1] || lim[1] > 255) { FAIL("case %ld: the table gave rc %d, limits %u %u", i, rc, lim[0], lim[1]); continue; }
			const uint8_t *t = lut.get() + 256 * p;
			for (int v = 1; v < 256; v++)
				if (t[v] < t[v - 1]) { FAIL("case %ld: the table falls at %d", i, v); break; }
			if (t[lim[0]] != 0 || t[lim[1]] != 255) FAIL("case %ld: the table is %u at lo and %u at hi", i, t[lim[0]], t[lim[1]]);
			if (lim[0] == 0 && lim[1] == 255) identity++; else stretched++;
		}
		/* ---- the model's render, sometimes through a map with entries beyond the line ---- */
		if (rng() % 5 == 0)
			for (int k = 0; k < 8; k++) map[rng() % width] = static_cast<uint32_t>(rng());
		const size_t out_bytes = static_cast<size_t>(8) * rows * width * planes, valid_bytes = static_cast<size_t>(rows) * width;
		auto out = exact<uint8_t>(out_bytes);
		auto valid = exact<uint8_t>(valid_bytes);
		const bool with_valid = rng() % 4 != 0;
		rc = mdemod_picture_model_render(image, filled, rows, select, planes, lut.get(), map.get(), width, out.get(), with_valid ? valid.get() : nullptr);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the render refused: %s", i, mdemod_last_error()); continue; }
		if (with_valid)
			for (size_t k = 0; k < valid_bytes; k++)
				if (valid[k] >> planes) { FAIL("case %ld: valid[%zu] = %u with %u planes", i, k, valid[k], planes); break; }
		if (mask_kind == 1)
			for (size_t k = 0; k < out_bytes; k++)
				if (out[k]) { FAIL("case %ld: a byte of a picture without a filled cell is %u", i, out[k]); break; }
		/* an argument out of range is refused before anything is touched */
		const uint32_t wrong[3] = { select[0], 3, select[2] };
		if (mdemod_picture_model_render(image, filled, rows, wrong, 3, lut.get(), map.get(), width, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_picture_model_render(image, filled, rows, select, 2, lut.get(), map.get(), width, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_picture_model_render(image, filled, rows, select, planes, lut.get(), map.get(), width + 2, nullptr, nullptr) != MDEMOD_ERR_PARAM)
			FAIL("case %ld: an argument out of range was accepted", i);
		/* ---- the whole-picture entry's model path: the pieces equal one batch ---- */
		mdemod_picture_result res, whole;
		rc = mdemod_picture_model_host(&o, image, filled, rows, select, planes, &res);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the host entry refused: %s", i, mdemod_last_error()); continue; }
		mdemod_picture_opts one = o;
		one.piece_rows = 65536;
		rc = mdemod_picture_model_host(&one, image, filled, rows, select, planes, &whole);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the host entry refused one batch: %s", i, mdemod_last_error()); mdemod_picture_free(&res); continue; }
		if (res.width != width || res.lines != 8 * rows || res.planes != planes || whole.width != width) FAIL("case %ld: the result is %u x %u x %u", i, res.width, res.lines, res.planes);
		else if (rows && (memcmp(res.pixels, whole.pixels, out_bytes) || memcmp(res.valid, whole.valid, valid_bytes) || memcmp(res.lo, whole.lo, sizeof res.lo) ||
		                  memcmp(res.hi, whole.hi, sizeof res.hi) || res.valid_cells != whole.valid_cells))
			FAIL("case %ld: pieces of %u rows change the picture", i, o.piece_rows);
		if (!rows && (res.pixels || res.valid)) FAIL("case %ld: an empty picture has pixels", i);
		if (res.valid_cells > valid_bytes) FAIL("case %ld: %llu valid cells of %zu", i, (unsigned long long)res.valid_cells, valid_bytes);
		if (!rows) empty++;
		if (planes == 3) colour++; else grey++;
		pieces++;
		mdemod_picture_free(&res);
		mdemod_picture_free(&whole);
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"refused\": %ld, \"empty\": %ld, \"grey\": %ld, \"colour\": %ld, \"stretched\": %ld, \"identity\": %ld, \"widths\": %zu, "
	       "\"pieces\": %ld, \"bad\": %ld}\n", bad ? "false" : "true", cases, refused, empty, grey, colour, stretched, identity, widths.size(), pieces, bad);
	return bad ? 1 : 0;
}
