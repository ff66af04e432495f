/*
 * fuzz_map.cpp — the host side of the map layer (csrc/map_host.cpp) under ASan + UBSan (tests/test_map_sanitize.py): the TLE parser
 * on mutated text (bytes changed, lines cut, lines doubled or dropped), the time fit on random placements and stamps, random options
 * (some out of range: refused with MDEMOD_ERR_PARAM and a text), grids of short passes anywhere on the orbit (polar ones are
 * refused), the forward function at the nodes, the model warp through the grid's nodes and through random ones, and the whole-map
 * entry's model path in bands of 16 .. 96 lines against one batch.  Every buffer is exactly as long as the interface says and comes
 * from the heap, so that one byte too far is a report.  What comes back is checked against the rules that hold for any input.
 * Prints one JSON line.
 * Usage: fuzz_map <cases> <seed> <tle file>
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/meteor_demod_amd_map.h"
#include "../../meteor_demod_amd/csrc/map_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

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
	long tle_ok = 0, tle_refused = 0, refused = 0, polar = 0, grids = 0, fits = 0, grey = 0, colour = 0, bands = 0, nodes_there = 0, nodes_missing = 0;
	for (long i = 0; i < cases; i++) {
		/* ---- the parser on mutated text: a copy on the heap that ends right behind its NUL ---- */
		for (int m = 0; m < 8; m++) {
			std::string t = text;
			switch (rng() % 6) {
			case 0: for (int k = 0; k < 1 + static_cast<int>(rng() % 3); k++) t[rng() % t.size()] = static_cast<char>(rng()); break;
			case 1: t.resize(rng() % (t.size() + 1)); break;
			case 2: t.erase(rng() % t.size(), 1 + rng() % 20); break;
			case 3: t.insert(rng() % t.size(), std::string(1 + rng() % 5, "12 \n-.9"[rng() % 7])); break;
			case 4: t += t; break;
			default: break;
			}
			for (char &c : t) if (!c) c = ' ';
			auto copy = exact<char>(t.size() + 1);
			memcpy(copy.get(), t.c_str(), t.size() + 1);
			mdemod_map_tle got;
			const int rc = mdemod_map_parse_tle(copy.get(), rng() % 4 ? 0 : 99001, &got);
			if (rc == MDEMOD_OK) {
				tle_ok++;
				if (!(got.mean_motion >= 0.5 && got.mean_motion <= 20.0) || !(got.inclination_deg >= 0.0 && got.inclination_deg <= 180.0) || !(got.eccentricity >= 0.0 && got.eccentricity < 1.0) ||
				    !(got.epoch_sec >= 0.0 && got.epoch_sec < 86400.0))
					FAIL("case %ld: an element set out of range was accepted", i);
			} else {
				tle_refused++;
				if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: the parser gave rc %d, text '%s'", i, rc, mdemod_last_error());
			}
		}
		/* ---- the packets of a short pass: random losses, some garbage stamps, sometimes nothing placed ---- */
		const uint32_t rows = 1 + static_cast<uint32_t>(rng() % 6);
		const double start = static_cast<double>(rng() % 86400000) / 1000.0, period = 1.0 + static_cast<double>(rng() % 500) / 1000.0;
		const int loss = static_cast<int>(rng() % 4);
		std::vector<mdemod_placement> pl;
		std::vector<mdemod_strip_info> si;
		for (uint32_t r = 0; r < rows; r++)
			for (int ch = 0; ch < 3; ch++)
				for (uint32_t c = 0; c < 14; c++) {
					if (loss == 3 || (loss && rng() % 3 == 0)) continue;
					const double s = fmod(start + r * period, 86400.0);
					mdemod_placement p = { rng() % 9 ? ch : -1, r, c, 0 };
					mdemod_strip_info q;
					memset(&q, 0, sizeof q);
					q.ms = rng() % 40 ? static_cast<uint32_t>(s * 1000.0) : static_cast<uint32_t>(rng());
					q.us = static_cast<uint16_t>(rng() % 40 ? 0 : rng());
					pl.push_back(p);
					si.push_back(q);
				}
		auto place = exact<mdemod_placement>(pl.size());
		auto sinfo = exact<mdemod_strip_info>(si.size());
		if (!pl.empty()) { memcpy(place.get(), pl.data(), pl.size() * sizeof pl[0]); memcpy(sinfo.get(), si.data(), si.size() * sizeof si[0]); }
		size_t placed = 0;
		for (const auto &p : pl) placed += p.channel >= 0;
		mdemod_map_opts o;
		mdemod_map_default_opts(&o);
		o.px_per_deg = 1.0 + static_cast<double>(rng() % 30);
		o.scan_deg = rng() & 1 ? 110.0 : 1.0 + static_cast<double>(rng() % 12901) / 100.0;
		o.side = rng() & 1 ? 1 : -1;
		o.stretch = rng() % 4 != 0;
		o.clip_low = static_cast<uint32_t>(rng() % 500);
		o.clip_high = static_cast<uint32_t>(rng() % 500);
		o.piece_lines = 16 * static_cast<uint32_t>(rng() % 7);
		if (rng() % 3 == 0) o.date = tle.epoch_day + static_cast<int32_t>(rng() % 5) - 2;
		bool broken = false;
		if (rng() % 8 == 0) {
			broken = true;
			switch (rng() % 7) {
			case 0: o.px_per_deg = rng() & 1 ? 0.5 : 1001.0; break;
			case 1: o.scan_deg = rng() & 1 ? 0.5 : 131.0; break;
			case 2: o.side = static_cast<int32_t>(rng() % 5) * 2; break;
			case 3: o.clip_low = 500 + static_cast<uint32_t>(rng() % 1000); break;
			case 4: o.piece_lines = 8 + 16 * static_cast<uint32_t>(rng() % 5); break;
			case 5: o.time_offset = NAN; break;
			default: o.row_period = rng() & 1 ? 0.0 : 11.0; break;
			}
		}
		mdemod_map_timing tm;
		int rc = mdemod_map_fit_time(place.get(), sinfo.get(), pl.size(), &o, &tm);
		if (broken || !placed) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: the fit of %s gave rc %d", i, broken ? "options out of range" : "no packet", rc);
			refused++;
			continue;
		}
		if (rc != MDEMOD_OK) {
			/* garbage stamps may leave no period within 0.1 .. 10 s: a refusal with a text */
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: the fit gave rc %d", i, rc);
			refused++;
			continue;
		}
		fits++;
		if (!(tm.row_period >= 0.1 && tm.row_period <= 10.0) || !(tm.s0 >= 0.0 && tm.s0 < 86400.0) || tm.lines > 8 * rows || tm.lines % 8 || !tm.lines || tm.placed != placed)
			FAIL("case %ld: the fit gave period %g, s0 %g, %u lines, %u placed of %zu", i, tm.row_period, tm.s0, tm.lines, tm.placed, placed);
		/* ---- the grid ---- */
		mdemod_map_nodes grid;
		rc = mdemod_map_grid(&tle, &tm, &o, 8 * rows, &grid);
		if (rc != MDEMOD_OK) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || grid.nodes) FAIL("case %ld: the grid gave rc %d, text '%s'", i, rc, mdemod_last_error());
			polar++;
			mdemod_map_result res;
			const uint32_t sel[3] = { 0, 1, 2 };
			auto img = exact<uint8_t>(rows * PIC_LINE_BYTES);
			auto fil = exact<uint8_t>(static_cast<size_t>(rows) * PIC_CELLS);
			memset(img.get(), 1, rows * PIC_LINE_BYTES);
			memset(fil.get(), 1, static_cast<size_t>(rows) * PIC_CELLS);
			const uint8_t *image[3] = { img.get(), img.get(), img.get() }, *filled[3] = { fil.get(), fil.get(), fil.get() };
			if (mdemod_map_model_host(&o, &tle, image, filled, rows, place.get(), sinfo.get(), pl.size(), sel, 3, &res) != MDEMOD_ERR_PARAM || res.pixels)
				FAIL("case %ld: the host entry took a pass whose grid is refused", i);
			continue;
		}
		grids++;
		const uint32_t W = grid.width, H = grid.height;
		if (W < 4 || W % 4 || W > MDEMOD_MAP_MAX_WIDTH || !H || H > MDEMOD_MAP_MAX_HEIGHT || grid.node_rows != map_node_count(H) || grid.node_cols != map_node_count(W) || !grid.sx ||
		    !(grid.lon_left >= -180.0 && grid.lon_left < 180.0) || !(fabs(grid.lat_top) <= 86.0))
			FAIL("case %ld: the grid is %u x %u, %u x %u nodes, sx %u, from %g %g", i, W, H, grid.node_rows, grid.node_cols, grid.sx, grid.lat_top, grid.lon_left);
		/* the nodes into a buffer of exactly their size; each one that is there maps back onto its point */
		const size_t n_nodes = static_cast<size_t>(grid.node_rows) * grid.node_cols;
		auto nodes = exact<int32_t>(2 * n_nodes);
		memcpy(nodes.get(), grid.nodes, 2 * n_nodes * sizeof(int32_t));
		mdemod_map_timing dated = tm;
		dated.date = grid.date;
		for (size_t k = 0; k < n_nodes; k++) {
			if (nodes[2 * k] == MDEMOD_MAP_NO_NODE && nodes[2 * k + 1] == MDEMOD_MAP_NO_NODE) { nodes_missing++; continue; }
			nodes_there++;
			const double y = nodes[2 * k + 1] / 256.0, x = nodes[2 * k] / 256.0;
			double lat, lon;
			if (mdemod_map_geolocate(&tle, &dated, &o, &y, &x, 1, &lat, &lon) != MDEMOD_OK || !std::isfinite(lat)) { FAIL("case %ld: node %zu is not visible", i, k); break; }
			const double want_lat = grid.lat_top - (16.0 * (k / grid.node_cols) + 0.5) / grid.sy, want_lon = grid.lon_left + (16.0 * (k % grid.node_cols) + 0.5) / grid.sx;
			const double d_lon = fmod(fabs(lon - want_lon), 360.0);
			/* a node is rounded to 1/256 pixel, a pixel is some 0.03 degree of longitude at worst below 85 degrees */
			if (fabs(lat - want_lat) > 1.0e-3 || std::min(d_lon, 360.0 - d_lon) > 1.0e-2) { FAIL("case %ld: node %zu maps to %g %g, its point is %g %g", i, k, lat, lon, want_lat, want_lon); break; }
		}
		/* ---- pictures and masks, each exactly as long as its rows; the model warp ---- */
		const uint32_t planes = rng() & 1 ? 3 : 1;
		const uint32_t select[3] = { static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3) };
		std::unique_ptr<uint8_t[]> img[3], fil[3];
		const uint8_t *image[3], *filled[3];
		for (int s = 0; s < 3; s++) {
			img[s] = exact<uint8_t>(rows * PIC_LINE_BYTES);
			fil[s] = exact<uint8_t>(static_cast<size_t>(rows) * PIC_CELLS);
			for (size_t k = 0; k < rows * PIC_LINE_BYTES; k++) img[s][k] = static_cast<uint8_t>(rng());
			for (size_t k = 0; k < static_cast<size_t>(rows) * PIC_CELLS; k++) fil[s][k] = static_cast<uint8_t>(rng() % 4 ? 1 + rng() % 255 : 0);
			image[s] = img[s].get();
			filled[s] = fil[s].get();
		}
		auto lut = exact<uint8_t>(256 * planes);
		for (size_t k = 0; k < 256 * planes; k++) lut[k] = static_cast<uint8_t>(rng());
		if (rng() % 3 == 0)
			for (int k = 0; k < 6; k++) nodes[rng() % (2 * n_nodes)] = static_cast<int32_t>(rng());      /* any int32 is a node */
		const size_t out_bytes = static_cast<size_t>(H) * W * planes, valid_bytes = static_cast<size_t>(H) * W;
		auto out = exact<uint8_t>(out_bytes);
		auto valid = exact<uint8_t>(valid_bytes);
		const bool with_valid = rng() % 4 != 0;
		rc = mdemod_map_model_warp(image, filled, rows, select, planes, lut.get(), nodes.get(), W, H, out.get(), with_valid ? valid.get() : nullptr);
		if (rc != MDEMOD_OK) FAIL("case %ld: the warp refused: %s", i, mdemod_last_error());
		else if (with_valid)
			for (size_t k = 0; k < valid_bytes; k++)
				if (valid[k] >> planes) { FAIL("case %ld: valid[%zu] = %u with %u planes", i, k, valid[k], planes); break; }
		const uint32_t wrong[3] = { select[0], 3, select[2] };
		if (mdemod_map_model_warp(image, filled, rows, wrong, 3, lut.get(), nodes.get(), W, H, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_map_model_warp(image, filled, rows, select, 2, lut.get(), nodes.get(), W, H, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_map_model_warp(image, filled, rows, select, planes, lut.get(), nodes.get(), W + 2, H, nullptr, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_map_model_warp(image, filled, rows, select, planes, lut.get(), nodes.get(), W, 16385, nullptr, nullptr) != MDEMOD_ERR_PARAM)
			FAIL("case %ld: an argument out of range was accepted", i);
		mdemod_map_grid_free(&grid);
		/* ---- the whole-map entry's model path: the bands equal one batch ---- */
		mdemod_map_result res, whole;
		rc = mdemod_map_model_host(&o, &tle, image, filled, rows, place.get(), sinfo.get(), pl.size(), select, planes, &res);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the host entry refused: %s", i, mdemod_last_error()); continue; }
		mdemod_map_opts one = o;
		one.piece_lines = MDEMOD_MAP_MAX_HEIGHT;
		rc = mdemod_map_model_host(&one, &tle, image, filled, rows, place.get(), sinfo.get(), pl.size(), select, planes, &whole);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the host entry refused one batch: %s", i, mdemod_last_error()); mdemod_map_free(&res); continue; }
		if (res.width != W || res.height != H || res.planes != planes || whole.width != W || whole.height != H) FAIL("case %ld: the result is %u x %u x %u", i, res.width, res.height, res.planes);
		else if (memcmp(res.pixels, whole.pixels, out_bytes) || memcmp(res.valid, whole.valid, valid_bytes) || memcmp(res.lo, whole.lo, sizeof res.lo) ||
		         memcmp(res.hi, whole.hi, sizeof res.hi) || res.valid_pixels != whole.valid_pixels)
			FAIL("case %ld: bands of %u lines change the map", i, o.piece_lines);
		if (res.valid_pixels > valid_bytes) FAIL("case %ld: %llu valid pixels of %zu", i, (unsigned long long)res.valid_pixels, valid_bytes);
		if (planes == 3) colour++; else grey++;
		bands++;
		mdemod_map_free(&res);
		mdemod_map_free(&whole);
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"tle_ok\": %ld, \"tle_refused\": %ld, \"refused\": %ld, \"polar\": %ld, \"fits\": %ld, \"grids\": %ld, \"grey\": %ld, "
	       "\"colour\": %ld, \"bands\": %ld, \"nodes_there\": %ld, \"nodes_missing\": %ld, \"bad\": %ld}\n", bad ? "false" : "true", cases, tle_ok, tle_refused,
	       refused, polar, fits, grids, grey, colour, bands, nodes_there, nodes_missing, bad);
	return bad ? 1 : 0;
}
