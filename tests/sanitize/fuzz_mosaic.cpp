/*
 * fuzz_mosaic.cpp — the host side of the mosaic layer (csrc/mosaic_host.cpp over csrc/map_host.cpp) under ASan + UBSan
 * (tests/test_mosaic_sanitize.py): 1 .. 8 passes of 1 .. 6 strip rows anywhere on the orbit, within seconds of each other so that
 * they overlap, random options (some out of range: refused with MDEMOD_ERR_PARAM and a text), the common grid (polar passes and passes without a placed packet are
 * refused), the model blend through the grid's nodes and through nodes of any int32, one pass against the map layer's model warp,
 * and the whole-mosaic entry's model path in bands of 16 .. 96 lines against one batch.  Every buffer is exactly as long as the
 * interface says and comes from the heap, so that one byte too far is a report.  What comes back is checked against the rules that
 * hold for any input.  Prints one JSON line.
 * Usage: fuzz_mosaic <cases> <seed> <tle file>
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/meteor_demod_amd_mosaic.h"
#include "../../meteor_demod_amd/csrc/mosaic_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

struct PassData {
	uint32_t rows = 0;
	size_t n_desc = 0, placed = 0;
	std::unique_ptr<mdemod_placement[]> place;
	std::unique_ptr<mdemod_strip_info[]> sinfo;
	std::unique_ptr<uint8_t[]> img[3], fil[3], lut;
	std::unique_ptr<int32_t[]> nodes;
	std::unique_ptr<char[]> text;
};

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 100;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	std::string text;
	if (FILE *f = argc > 3 ? fopen(argv[3], "rb") : nullptr) {
		char block[512];
		for (size_t n; (n = fread(block, 1, sizeof block, f)) > 0;) text.append(block, n);
		fclose(f);
	}
	mdemod_map_tle tle;
	if (mdemod_map_parse_tle(text.c_str(), 0, &tle) != MDEMOD_OK) { fprintf(stderr, "the element set of %s is not read: %s\n", argc > 3 ? argv[3] : "(none)", mdemod_last_error()); return 2; }
	long refused = 0, grid_refused = 0, grids = 0, passes_total = 0, grey = 0, colour = 0, bands = 0, feather = 0, best = 0, wild = 0, single = 0, overlap = 0, most = 0;
	for (long i = 0; i < cases; i++) {
		const uint32_t n = 1 + static_cast<uint32_t>(rng() % 8);
		const double start = static_cast<double>(rng() % 86400000) / 1000.0;
		std::vector<PassData> data(n);
		auto passes = exact<mdemod_mosaic_pass>(n);
		memset(passes.get(), 0, n * sizeof(mdemod_mosaic_pass));
		const int loss = static_cast<int>(rng() % 8);                                   /* 7: one pass of the case has nothing placed */
		const uint32_t unlucky = static_cast<uint32_t>(rng() % n);
		bool nothing_placed = false;
		for (uint32_t k = 0; k < n; k++) {
			PassData &d = data[k];
			d.rows = 1 + static_cast<uint32_t>(rng() % 6);
			const double s0 = start + static_cast<double>(rng() % 120) / 10.0, period = 1.0 + static_cast<double>(rng() % 500) / 1000.0;
			std::vector<mdemod_placement> pl;
			std::vector<mdemod_strip_info> si;
			for (uint32_t r = 0; r < d.rows; r++)
				for (int ch = 0; ch < 3; ch++)
					for (uint32_t c = 0; c < 14; c++) {
						if ((loss == 7 && k == unlucky) || (loss % 3 == 1 && rng() % 3 == 0)) continue;
						const double s = fmod(s0 + r * period, 86400.0);
						mdemod_placement p = { rng() % 9 ? ch : -1, r, c, 0 };
						mdemod_strip_info q;
						memset(&q, 0, sizeof q);
						q.ms = rng() % 40 ? static_cast<uint32_t>(s * 1000.0) : static_cast<uint32_t>(rng());
						pl.push_back(p);
						si.push_back(q);
					}
			d.n_desc = pl.size();
			d.place = exact<mdemod_placement>(pl.size());
			d.sinfo = exact<mdemod_strip_info>(si.size());
			if (!pl.empty()) { memcpy(d.place.get(), pl.data(), pl.size() * sizeof pl[0]); memcpy(d.sinfo.get(), si.data(), si.size() * sizeof si[0]); }
			for (const auto &p : pl) d.placed += p.channel >= 0;
			nothing_placed = nothing_placed || !d.placed;
			d.text = exact<char>(text.size() + 1);
			memcpy(d.text.get(), text.c_str(), text.size() + 1);
			for (int s = 0; s < 3; s++) {
				d.img[s] = exact<uint8_t>(d.rows * PIC_LINE_BYTES);
				d.fil[s] = exact<uint8_t>(static_cast<size_t>(d.rows) * PIC_CELLS);
				for (size_t b = 0; b < d.rows * PIC_LINE_BYTES; b++) d.img[s][b] = static_cast<uint8_t>(rng());
				for (size_t b = 0; b < static_cast<size_t>(d.rows) * PIC_CELLS; b++) d.fil[s][b] = static_cast<uint8_t>(rng() % 4 ? 1 + rng() % 255 : 0);
			}
			mdemod_mosaic_pass &p = passes[k];
			p.tle_text = d.text.get();
			p.norad = rng() % 4 ? 0 : tle.norad;
			p.date = rng() % 3 ? MDEMOD_MOSAIC_DATE_AUTO : tle.epoch_day + static_cast<int32_t>(rng() % 5) - 2;
			for (int s = 0; s < 3; s++) { p.image[s] = d.img[s].get(); p.filled[s] = d.fil[s].get(); }
			p.rows = d.rows; p.place = d.place.get(); p.sinfo = d.sinfo.get(); p.n_desc = d.n_desc;
		}
		mdemod_mosaic_opts o;
		mdemod_mosaic_default_opts(&o);
		o.px_per_deg = 1.0 + static_cast<double>(rng() % 8);
		o.scan_deg = rng() & 1 ? 110.0 : 1.0 + static_cast<double>(rng() % 12901) / 100.0;
		o.side = rng() & 1 ? 1 : -1;
		o.stretch = static_cast<uint32_t>(rng() % 3);
		o.clip_low = static_cast<uint32_t>(rng() % 500);
		o.clip_high = static_cast<uint32_t>(rng() % 500);
		o.piece_lines = 16 * static_cast<uint32_t>(rng() % 7);
		o.blend = static_cast<uint32_t>(rng() & 1);
		const uint32_t planes = rng() & 1 ? 3 : 1;
		const uint32_t select[3] = { static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3) };
		mdemod_mosaic_nodes grid;
		mdemod_mosaic_result res, whole;
		if (rng() % 8 == 0) {
			uint32_t count = n;
			switch (rng() % 9) {
			case 0: o.px_per_deg = rng() & 1 ? 0.5 : 1001.0; break;
			case 1: o.scan_deg = rng() & 1 ? 0.5 : 131.0; break;
			case 2: o.side = static_cast<int32_t>(rng() % 5) * 2; break;
			case 3: o.clip_low = 500 + static_cast<uint32_t>(rng() % 1000); break;
			case 4: o.piece_lines = 8 + 16 * static_cast<uint32_t>(rng() % 5); break;
			case 5: o.time_offset = NAN; break;
			case 6: o.stretch = 3 + static_cast<uint32_t>(rng() % 5); break;
			case 7: o.blend = 2 + static_cast<uint32_t>(rng() % 5); break;
			default: count = rng() & 1 ? 0 : 9; break;                                 /* (refused before a ninth pass is looked at) */
			}
			const int rc = mdemod_mosaic_grid(&o, passes.get(), count, &grid);
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || grid.nodes[0]) FAIL("case %ld: options out of range gave rc %d, text '%s'", i, rc, mdemod_last_error());
			if (mdemod_mosaic_model_host(&o, passes.get(), count, select, planes, &res) != MDEMOD_ERR_PARAM || res.pixels) FAIL("case %ld: the host entry took options out of range", i);
			refused++;
			continue;
		}
		/* ---- the common grid ---- */
		int rc = mdemod_mosaic_grid(&o, passes.get(), n, &grid);
		if (rc != MDEMOD_OK) {
			/* a polar pass, nothing placed, or garbage stamps that leave no period: a refusal with a text, and nothing handed out */
			bool any = false;
			for (int k = 0; k < MDEMOD_MOSAIC_MAX_PASSES; k++) any = any || grid.nodes[k];
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || any) FAIL("case %ld: the grid gave rc %d, text '%s'", i, rc, mdemod_last_error());
			if (mdemod_mosaic_model_host(&o, passes.get(), n, select, planes, &res) != MDEMOD_ERR_PARAM || res.pixels) FAIL("case %ld: the host entry took passes whose grid is refused", i);
			grid_refused++;
			continue;
		}
		if (nothing_placed) FAIL("case %ld: a pass without a placed packet was accepted", i);
		grids++;
		passes_total += n;
		most = n > most ? n : most;
		const uint32_t W = grid.width, H = grid.height;
		if (W < 4 || W % 4 || W > MDEMOD_MOSAIC_MAX_WIDTH || !H || H > MDEMOD_MOSAIC_MAX_HEIGHT || grid.node_rows != map_node_count(H) || grid.node_cols != map_node_count(W) ||
		    !grid.sx || grid.n != n || !(grid.lon_left >= -180.0 && grid.lon_left < 180.0) || !(fabs(grid.lat_top) <= 86.0))
			FAIL("case %ld: the grid is %u x %u, %u x %u nodes, sx %u, from %g %g", i, W, H, grid.node_rows, grid.node_cols, grid.sx, grid.lat_top, grid.lon_left);
		const size_t n_nodes = static_cast<size_t>(grid.node_rows) * grid.node_cols;
		const bool any_int = rng() % 3 == 0;
		wild += any_int;
		auto sources = exact<mdemod_mosaic_source>(n);
		memset(sources.get(), 0, n * sizeof(mdemod_mosaic_source));
		for (uint32_t k = 0; k < n; k++) {
			PassData &d = data[k];
			if (grid.timing[k].lines != 8 * d.rows || !(grid.timing[k].row_period >= 0.1 && grid.timing[k].row_period <= 10.0) || grid.timing[k].date == MDEMOD_MOSAIC_DATE_AUTO)
				FAIL("case %ld: pass %u has %u lines, period %g, date %d", i, k, grid.timing[k].lines, grid.timing[k].row_period, grid.timing[k].date);
			d.nodes = exact<int32_t>(2 * n_nodes);
			memcpy(d.nodes.get(), grid.nodes[k], 2 * n_nodes * sizeof(int32_t));
			if (any_int)
				for (int m = 0; m < 6; m++) d.nodes[rng() % (2 * n_nodes)] = static_cast<int32_t>(rng());      /* any int32 is a node */
			d.lut = exact<uint8_t>(256 * planes);
			for (size_t b = 0; b < 256 * planes; b++) d.lut[b] = static_cast<uint8_t>(rng());
			mdemod_mosaic_source &s = sources[k];
			for (int c = 0; c < 3; c++) { s.image[c] = d.img[c].get(); s.filled[c] = d.fil[c].get(); }
			s.lut = d.lut.get(); s.nodes = d.nodes.get();
			s.rows = n > 1 && rng() % 16 == 0 ? 0 : d.rows;                            /* sometimes an empty pass */
		}
		mdemod_mosaic_grid_free(&grid);
		/* ---- the model blend into buffers of exactly their sizes ---- */
		const size_t out_bytes = static_cast<size_t>(H) * W * planes, area = static_cast<size_t>(H) * W;
		auto out = exact<uint8_t>(out_bytes);
		auto valid = exact<uint8_t>(area);
		auto cover = exact<uint8_t>(area);
		const bool with_valid = rng() % 4 != 0, with_cover = rng() % 4 != 0;
		rc = mdemod_mosaic_model_blend(sources.get(), n, select, planes, o.blend, W, H, out.get(), with_valid ? valid.get() : nullptr, with_cover ? cover.get() : nullptr);
		if (rc != MDEMOD_OK) FAIL("case %ld: the blend refused: %s", i, mdemod_last_error());
		else {
			for (size_t b = 0; with_valid && b < area; b++)
				if (valid[b] >> planes) { FAIL("case %ld: valid[%zu] = %u with %u planes", i, b, valid[b], planes); break; }
			for (size_t b = 0; with_cover && b < area; b++) {
				if (cover[b] >> n) { FAIL("case %ld: cover[%zu] = %u with %u passes", i, b, cover[b], n); break; }
				if (with_valid && !cover[b] != !valid[b]) { FAIL("case %ld: cover[%zu] = %u and valid = %u", i, b, cover[b], valid[b]); break; }
				overlap += (cover[b] & (cover[b] - 1)) != 0;
			}
		}
		if (n == 1 && rc == MDEMOD_OK) {
			/* one pass: the map layer's warp, in both modes */
			auto one = exact<uint8_t>(out_bytes);
			auto one_valid = exact<uint8_t>(area);
			const uint8_t *image[3] = { sources[0].image[0], sources[0].image[1], sources[0].image[2] }, *filled[3] = { sources[0].filled[0], sources[0].filled[1], sources[0].filled[2] };
			if (mdemod_map_model_warp(image, filled, sources[0].rows, select, planes, sources[0].lut, sources[0].nodes, W, H, one.get(), one_valid.get()) != MDEMOD_OK ||
			    memcmp(one.get(), out.get(), out_bytes) || (with_valid && memcmp(one_valid.get(), valid.get(), area)))
				FAIL("case %ld: one pass is not the map layer's warp", i);
			single++;
		}
		const uint32_t wrong[3] = { select[0], 3, select[2] };
		if (mdemod_mosaic_model_blend(sources.get(), n, wrong, 3, o.blend, W, H, nullptr, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_mosaic_model_blend(sources.get(), n, select, 2, o.blend, W, H, nullptr, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_mosaic_model_blend(sources.get(), 9, select, planes, o.blend, W, H, nullptr, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_mosaic_model_blend(sources.get(), n, select, planes, 2, W, H, nullptr, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_mosaic_model_blend(sources.get(), n, select, planes, o.blend, W + 2, H, nullptr, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_mosaic_model_blend(sources.get(), n, select, planes, o.blend, W, 16385, nullptr, nullptr, nullptr) != MDEMOD_ERR_PARAM)
			FAIL("case %ld: an argument out of range was accepted", i);
		/* ---- the whole-mosaic entry's model path: the bands equal one batch ---- */
		rc = mdemod_mosaic_model_host(&o, passes.get(), n, select, planes, &res);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the host entry refused: %s", i, mdemod_last_error()); continue; }
		mdemod_mosaic_opts one = o;
		one.piece_lines = MDEMOD_MOSAIC_MAX_HEIGHT;
		rc = mdemod_mosaic_model_host(&one, passes.get(), n, select, planes, &whole);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the host entry refused one batch: %s", i, mdemod_last_error()); mdemod_mosaic_free(&res); continue; }
		if (res.width != W || res.height != H || res.planes != planes || res.n != n || whole.width != W || whole.height != H)
			FAIL("case %ld: the result is %u x %u x %u of %u passes", i, res.width, res.height, res.planes, res.n);
		else if (memcmp(res.pixels, whole.pixels, out_bytes) || memcmp(res.valid, whole.valid, area) || memcmp(res.cover, whole.cover, area) || memcmp(res.lo, whole.lo, sizeof res.lo) ||
		         memcmp(res.hi, whole.hi, sizeof res.hi) || res.valid_pixels != whole.valid_pixels || res.overlap_pixels != whole.overlap_pixels ||
		         memcmp(res.covered, whole.covered, sizeof res.covered))
			FAIL("case %ld: bands of %u lines change the mosaic", i, o.piece_lines);
		if (res.valid_pixels > area || res.overlap_pixels > res.valid_pixels) FAIL("case %ld: %llu valid and %llu overlapping pixels of %zu", i, (unsigned long long)res.valid_pixels,
		                                                                           (unsigned long long)res.overlap_pixels, area);
		if (planes == 3) colour++; else grey++;
		if (o.blend) best++; else feather++;
		bands++;
		mdemod_mosaic_free(&res);
		mdemod_mosaic_free(&whole);
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"refused\": %ld, \"grid_refused\": %ld, \"grids\": %ld, \"passes\": %ld, \"most\": %ld, \"grey\": %ld, \"colour\": %ld, \"feather\": %ld, "
	       "\"best\": %ld, \"bands\": %ld, \"wild\": %ld, \"single\": %ld, \"overlap\": %ld, \"bad\": %ld}\n", bad ? "false" : "true", cases, refused, grid_refused, grids,
	       passes_total, most, grey, colour, feather, best, bands, wild, single, overlap, bad);
	return bad ? 1 : 0;
}
